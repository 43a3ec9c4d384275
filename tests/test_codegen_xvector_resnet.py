"""The kernels of the ResNet x-vector extractor (csrc/conv2d.hip) in the built library's gfx950 code object: present, without scratch
memory and without spilled registers (no GPU; the metadata reader of tests/test_codegen_invariants.py).  conv2d_mfma_kernel keeps up to
32 accumulators per lane across a fully unrolled tap loop; all eight instantiations (3x3 / 1x1, stride 1 / 2, 32 / 64 output channels
per block) must be there."""
from test_codegen_invariants import code_objects  # noqa: F401  (the module-scoped fixture)

KERNELS = {"conv2d_mfma_kernel": 8, "conv2d_stem_kernel": 1, "se_scale_add_relu_kernel": 1, "row_mean_std_kernel": 1}


def test_resnet_kernels_have_no_scratch_and_no_spills(code_objects):  # noqa: F811
    meta = code_objects["meta"]
    for name, count in KERNELS.items():
        syms = [k for k in meta if name in k]
        assert len(syms) == count, (name, syms)
        for sym in syms:
            assert meta[sym]["scratch"] == 0 and meta[sym]["vgpr_spill_count"] == 0, (sym, meta[sym])
