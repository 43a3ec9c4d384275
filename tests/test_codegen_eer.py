"""Both instantiations of eer_bootstrap_kernel (csrc/stats/eer_bootstrap.hip: a wave per replicate, a block per replicate) in the built
library's gfx950 code object: present, without scratch memory and without spilled registers (no GPU; the metadata reader of
tests/test_codegen_invariants.py).  The kernel regenerates a replicate's draws in every sweep precisely so that nothing of it lives in
memory: draws kept in a per-thread array would show here as scratch."""
from test_codegen_invariants import code_objects  # noqa: F401  (the module-scoped fixture)


def test_eer_bootstrap_kernel_has_no_scratch_and_no_spills(code_objects):  # noqa: F811
    meta = code_objects["meta"]
    syms = sorted(k for k in meta if "eer_bootstrap_kernel" in k)
    assert len(syms) == 2 and "ILb0E" in syms[0] and "ILb1E" in syms[1], syms
    for sym in syms:
        assert meta[sym]["scratch"] == 0 and meta[sym]["vgpr_spill_count"] == 0, (sym, meta[sym])
