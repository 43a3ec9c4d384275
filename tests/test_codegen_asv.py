"""The three ASV scoring kernels (csrc/asv_score.hip) in the built library's gfx950 code object: present, without scratch memory
and without spilled registers (no GPU; the metadata reader of tests/test_codegen_invariants.py).  cohort_topk_stats_kernel keeps
64 accumulators per lane in statically indexed registers: a dynamic index would put them in scratch, which this check would see."""
from test_codegen_invariants import code_objects  # noqa: F401  (the module-scoped fixture)

KERNELS = ("cohort_topk_stats_kernel", "trial_scores_kernel", "segment_mean_l2norm_kernel")


def test_asv_kernels_have_no_scratch_and_no_spills(code_objects):  # noqa: F811
    meta = code_objects["meta"]
    for name in KERNELS:
        syms = [k for k in meta if name in k]
        assert len(syms) == 1, (name, syms)
        for sym in syms:
            assert meta[sym]["scratch"] == 0 and meta[sym]["vgpr_spill_count"] == 0, (sym, meta[sym])
