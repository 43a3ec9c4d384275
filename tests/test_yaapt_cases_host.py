"""The input catalogue of the YAAPT stage tests (tests/yaapt_cases.py) keeps its proven properties: frame counts, frames
above the NLFER threshold, frames with a spectral candidate (`nv`), a NaN `pitch_std`, a NaN `mean_pitch`, the raises —
asserted from the float32 oracle's intermediates, so that a case which drifts off its edge fails here and not silently on
the device.  Also: the share of frames whose float32 decisions the float64 references exempt stays inside the caps the
device test applies.  CPU only."""
import pytest
import torch

import yaapt_cases as yc
from oracle import yaapt as oy
from test_ref64_yaapt import ANY_ORDER


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("case", [c for c in yc.CASES if not c.refused], ids=repr)
def test_case_has_its_properties(case):
    aux, final, raised = yc.oracle_run(case)
    got = yc.check_properties(case, aux)
    assert raised == (case.raises or ""), (case, raised)
    if case.raises:
        assert got["nv"] == 0 and got["vuv"] > 0          # frames above the threshold, none with a candidate
    else:
        assert final.shape == (case.nframes,)


def test_catalogue_covers_the_edges():
    acc = yc.accepted()
    nf = {c.nframes for c in acc}
    assert {4, 5, 63, 64, 65, 66, 128, 129, 130, 256, 258, 2048} <= nf
    assert {62, 63, 64, 65, 127, 128, 129, 255, 256} <= {c.vuv for c in acc}
    assert {1, 2, 3, 4, 64, 65, 128, 256} <= {c.nv for c in acc}
    assert any(c.underflows for c in acc) and any(c.kind == "burst" and not c.underflows and c.nv == 2 for c in acc)
    assert any(c.std_nan for c in acc) and any(c.mean_nan for c in acc)
    assert {c.nframes for c in yc.refused()} == {yc.MIN_FRAMES - 1, yc.MAX_FRAMES + 1}
    assert len(yc.raising()) >= 3 and {c.kind for c in acc} == {"tone", "burst", "noise", "clip"}
    assert all(c.n <= 82241 for c in acc if not c.exact_only)
    for c in yc.CASES:
        assert oy.Plan(c.n, yc.OPTS).nframes == c.nframes, c


def test_refused_lengths_are_outside_the_entry_points_range():
    for c in yc.refused():
        assert not yc.MIN_FRAMES <= c.nframes <= yc.MAX_FRAMES


@pytest.mark.parametrize("case", [c for c in yc.accepted() if not c.exact_only], ids=repr)
def test_float32_decisions_stay_inside_the_exemption_caps(case):
    """the float32 oracle judged the way the device is: decisions equal to the float64 ones wherever the margin clears
    the bound, and the exempted frames within the cap (none on the gated tones, 1 % on noise and the clipped tone)"""
    res = yc.judged_oracle(case, ANY_ORDER)
    for stage, r in res.items():
        assert not r.get("wrong"), (case, stage, r["wrong"][:4])
    yc.assert_exempt_cap(case, res, yc.oracle_run(case)[0]["energy"])
