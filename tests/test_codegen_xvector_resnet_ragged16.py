"""The instantiations of conv2d_segments_f16x3_kernel (csrc/ragged2d16/conv2d_f16x3_segments.hip) in the built library's gfx950 code object:
present in the count the source declares (R16_KERNELS) and for the tiles its entry point dispatches to, which are the per-call kernel's
(csrc/conv2d16/conv2d_f16x3.hip), without scratch memory and without spilled registers (no GPU; the metadata reader of
tests/test_codegen_invariants.py).  Like the per-call kernel it keeps a chunk's staged elements and up to four accumulator tiles in
registers: a spill would put them in scratch memory behind every MFMA phase."""
import os
import re

from test_codegen_invariants import code_objects  # noqa: F401  (the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "conv2d_segments_f16x3_kernel"


def test_conv2d_segments_f16x3_kernels_are_present_without_scratch_and_spills(code_objects):  # noqa: F811
    text = open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "ragged2d16", "conv2d_f16x3_segments.hip")).read()
    declared = int(re.search(r"constexpr int R16_KERNELS = (\d+);", text).group(1))
    dispatched = set(re.findall(r"SAT_R16\((\d), (\d), (\d), (\d)\)", text))
    assert len(dispatched) == declared == 6
    # the tile choice is the per-call kernel's
    per_call = open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "conv2d16", "conv2d_f16x3.hip")).read()
    assert dispatched == set(re.findall(r"SAT_C16\((\d), (\d), (\d), (\d)\)", per_call))
    meta = code_objects["meta"]
    syms = sorted(k for k in meta if re.match(rf"_ZN3sat\d+{KERNEL}I", k))
    assert len(syms) == declared, syms
    for ks, s, mt, nt in dispatched:
        assert any(f"ILi{ks}ELi{s}ELi{mt}ELi{nt}E" in k for k in syms), (ks, s, mt, nt, syms)
    for sym in syms:
        assert meta[sym]["scratch"] == 0 and meta[sym]["vgpr_spill_count"] == 0, (sym, meta[sym])
    # the names the other components' tests count by substring stay theirs
    for other in ("conv2d_f16x3_kernel", "conv2d_mfma_kernel", "conv2d_segments_mfma_kernel", "conv2d_stem_kernel"):
        assert other not in KERNEL
