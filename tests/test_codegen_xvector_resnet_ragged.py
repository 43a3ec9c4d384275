"""The kernels of csrc/ragged2d/ in the built library's gfx950 code object (no GPU), read with the metadata reader of
tests/test_codegen_invariants.py: each is present with the expected number of instantiations, uses no scratch and spills no register.
Nothing else about the code is checked."""
import re

from test_codegen_invariants import code_objects  # noqa: F401  (the fixture)

# kernel -> instantiations: the MFMA conv over (ksize 3 | 1) x (stride 1 | 2) x (32 | 64 output channels per block)
KERNELS = {"conv2d_segments_mfma_kernel": 8, "conv2d_segments_stem_kernel": 1, "plane_mean_segments_kernel": 1,
           "se_scale_add_relu_segments_kernel": 1, "row_mean_std_segments_kernel": 1}


def test_the_ragged2d_kernels_are_in_the_code_object_without_scratch_or_spills(code_objects):  # noqa: F811
    meta = code_objects["meta"]
    for kernel, count in KERNELS.items():
        found = {sym: m for sym, m in meta.items() if re.match(rf"_ZN3sat\d+{kernel}(I|E)", sym)}
        assert len(found) == count, (kernel, sorted(found))
        for sym, m in found.items():
            assert m["scratch"] == 0 and m["vgpr_spill_count"] == 0, (sym, m)
    conv = sorted(re.search(r"ILi(\d)ELi(\d)ELi(\d)E", s).groups() for s in meta if "conv2d_segments_mfma_kernel" in s)
    assert conv == sorted((str(k), str(s), str(mt)) for k in (3, 1) for s in (1, 2) for mt in (1, 2))
