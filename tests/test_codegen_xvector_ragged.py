"""The segment kernels of the ragged x-vector batches (csrc/ragged/xvector_ragged.hip) in the built library's gfx950 code object: present, both
instantiations of the chain, without scratch memory and without spilled registers (no GPU; the metadata reader of
tests/test_codegen_invariants.py).  The chain keeps its weights, the next piece's input and NT accumulator tiles in registers like
res2_chain_kernel does: it must not pay for the segment table with spills."""
from test_codegen_invariants import code_objects  # noqa: F401  (the module-scoped fixture)

KERNELS = {"melspec_logmel_segments_kernel": 1, "instnorm_segments_kernel": 1, "row_mean_segments_kernel": 1, "se_gate_add_segments_kernel": 1,
           "attentive_stats_segments_kernel": 1, "res2_chain_segments_kernel": 2}


def test_segment_kernels_have_no_scratch_and_no_spills(code_objects):  # noqa: F811
    meta = code_objects["meta"]
    for name, count in KERNELS.items():
        syms = [k for k in meta if name in k]
        assert len(syms) == count, (name, syms)
        for sym in syms:
            assert meta[sym]["scratch"] == 0 and meta[sym]["vgpr_spill_count"] == 0, (sym, meta[sym])

