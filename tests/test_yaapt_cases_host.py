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


# ---- the option sets ---------------------------------------------------------------------------------------------------
def test_option_sets_sit_on_their_declared_edges():
    """the plan fields each set names, from oracle.yaapt.Plan; the device's limits restated for the sets it must accept"""
    names = [s.name for s in yc.OPTION_SETS]
    assert len(set(names)) == len(names)
    for s in yc.OPTION_SETS:
        plan = oy.Plan(s.cases[0].n, s.opts)
        got = dict(vars(plan), ov=plan.tda_len - plan.frame_jump)
        for key, want in s.fields.items():
            assert got[key] == want, (s, key, got[key], want)
        if s.refused:
            continue
        for c in s.cases:
            p = oy.Plan(c.n, s.opts)
            assert yc.MIN_FRAMES <= p.nframes <= yc.MAX_FRAMES and p.tda_nframes == p.nframes and p.need >= p.L, c
            assert p.nframe_size <= 1280 and p.max_shc <= 256 and p.max_shc * (p.nharm + 1) + p.wl <= 1280, c
            assert p.frame_jump < p.tda_len <= 1024 and p.tda_len - p.frame_jump <= 128 and p.median_value in (1, 3, 5, 7), c
    limits = {s.name: oy.Plan(s.cases[0].n, s.opts) for s in yc.accepted_sets()}
    assert any(p.nframe_size == 1280 and p.tda_len - p.frame_jump == 128 for p in limits.values())
    assert any(p.tda_len == 1024 for p in limits.values()) and any(p.tda_len - p.frame_jump == 1 for p in limits.values())
    assert {1, 3, 4, 6} <= {p.nharm for p in limits.values()} and {1, 3, 5, 7} <= {p.median_value for p in limits.values()}
    assert {8000.0, 16000.0, 22050.0} <= {p.fs for p in limits.values()}
    # the largest harmonic count: one more does not fit the magnitude window at this set's max_shc
    p = limits["nharm6_f0max250"]
    assert p.max_shc * (p.nharm + 2) + p.wl > 1280
    # lane edges per set: a frame count of 63, 64 or 65 (or 128 / 129) among the signals of every set that moves the jump
    for name in ("jump512_ov128", "tda1024", "ov1", "short", "sr8000", "sr22050"):
        assert {c.nframes for c in yc.option_set(name).cases} & {63, 64, 65, 128, 129}, name


def test_every_option_key_is_moved_by_some_device_test():
    """every key of DEFAULTS is off its default in a set the device runs, or in a refusal: a key added later cannot go untested"""
    from satools_amd import f0
    assert f0.DEFAULTS == oy.DEFAULTS
    moved = set()
    for s in yc.OPTION_SETS:
        moved |= {k for k, v in s.opts.items() if float(v) != f0.DEFAULTS[k]}
    assert moved == set(f0.DEFAULTS), sorted(set(f0.DEFAULTS) - moved)
    scalars = ("nlfer_thresh1", "nlfer_thresh2", "shc_thresh1", "shc_thresh2", "f0_double", "f0_half", "dp5_k1", "nccf_thresh1", "nccf_thresh2",
               "merit_boost", "merit_pivot", "merit_extra", "dp_w1", "dp_w2", "dp_w3", "dp_w4", "spec_pitch_min_std")
    wired = {s.wiring[0]: s for s in yc.OPTION_SETS if s.wiring}
    assert sorted(wired) == sorted(scalars)
    for key, s in wired.items():
        assert {k for k in s.opts if s.opts[k] != yc.OPTS.get(k)} == {key}, s          # that key alone, against OPTS


# what tests/test_hip_yaapt_stages.py::check_every_stage compares with the device: a wiring set may be observed through these only
DEVICE_COMPARES = ("vuv", "cand_pitch", "cand_merit", "spec_pitch", "pitch_std", "tp1+tp2", "ref_pitch", "ref_merit", "final")


def _observed(aux, final, what):
    assert what in DEVICE_COMPARES, what
    if what == "final":
        return final
    if what == "tp1+tp2":
        return torch.cat((aux["tp1"], aux["tp2"]))
    return aux[what].float()


@pytest.mark.parametrize("s", [s for s in yc.OPTION_SETS if s.wiring], ids=repr)
def test_wiring_set_changes_what_the_oracle_returns(s):
    """the set's one option, on the set's signal, changes the named intermediate (or the final track) of the float32 oracle against
    the unchanged options: a kernel that ignores the option cannot pass the device test of this pair"""
    case = s.cases[0]
    aux, final, raised = yc.oracle_run(case)
    base_aux = {}
    base = oy.yaapt_one(case.wav(), yc.OPTS, aux=base_aux)
    assert raised == ""
    a, b = _observed(aux, final, s.wiring[1]), _observed(base_aux, base, s.wiring[1])
    assert a.shape == b.shape and not torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)), s


def test_median_sets_change_the_track():
    """on the noisy signal of each median set the oracle's final track differs from that of every other width, and its spectral pitch
    from that of every other width of spec_track's own median (max(1, median_value - 2)): a kernel with a hard-coded width fails the device test of that pair.  (Found by a
    mutation check: with a clean and a clipped tone only, a refine kernel with the width fixed at 7 passed medians 3 and 5.)"""
    for m in (1, 3, 5):
        case = yc.option_set(f"median{m}").cases[-1]
        assert case.kind == "noise"
        aux, final, raised = yc.oracle_run(case)
        assert raised == ""
        for other in (1, 3, 5, 7):
            if other != m:
                b = {}
                f = oy.yaapt_one(case.wav(), {**yc.OPTS, "median_value": float(other)}, aux=b)
                assert not torch.equal(f, final), (m, other)
                assert torch.equal(b["spec_pitch"], aux["spec_pitch"]) == (max(1, other - 2) == max(1, m - 2)), (m, other)


@pytest.mark.parametrize("case", yc.option_cases(), ids=repr)
def test_float32_decisions_stay_inside_the_exemption_caps_under_every_option_set(case):
    """as above with the set's plan: no exempt frame on the tones and bursts, at most 1 % of the frames on the noisy and clipped ones"""
    plan = oy.Plan(case.n, case.opts)
    res = yc.judged_oracle(case, yc.any_order(plan))
    for stage, r in res.items():
        assert not r.get("wrong"), (case, stage, r["wrong"][:4])
    yc.assert_exempt_cap(case, res, yc.oracle_run(case)[0]["energy"])
