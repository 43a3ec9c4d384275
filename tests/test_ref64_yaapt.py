"""The float64 restatements of the YAAPT stages (tests/ref64_yaapt.py) pinned against the float32 oracle
(oracle/yaapt.py, itself bit-exact against the reference's tracks): on fixture utterances and on the edge catalogue every
value agrees within the derived bound and every decision is equal wherever its float64 margin clears the bound.  Then
the judges are shown to bite: a shifted lag, a rescaled energy, a dropped peak turn them red.  CPU only.

ROUNDINGS OF THE ORACLE.  torch's CPU reductions (sum, mean, matmul, the rfft of pocketfft) keep their order to themselves,
so every sum is given the count that holds for ANY order: n terms collect at most n - 1 additions, plus one for the product
or the division around them.  The FFT is judged by the running radix-2 bound of ref64_yaapt (its stated assumption on
mixed-radix passes).  |X| of a complex64 is hypotf: 1 ULP = 2 U tabulated, 2 ULP budgeted."""
import numpy as np
import pytest
import torch

import ref64_yaapt as r64
import yaapt_cases as yc
from oracle import yaapt as oy
from satools_amd import synthetic

ANY_ORDER = r64.Roundings(cmul=3.25, hyp=4, nl_sum=lambda n: n, en_mean=lambda n: n, sp_mean=lambda n: n + 1,
                          shc_sum=lambda n: n, shc_avg=lambda n: n, fm_head=lambda n: 401, fm_tail=lambda n: 400,
                          dot=lambda n: n + 1, pw=lambda n: n + 1)
PIN_CASES = [c for c in yc.accepted() if not c.exact_only]


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _assert_pinned(name, res):
    for stage, r in res.items():
        assert not r.get("wrong"), (name, stage, r["wrong"][:4])
        assert r["ratio"] <= 1.0, (name, stage, r["ratio"])


@pytest.mark.parametrize("case", PIN_CASES, ids=repr)
def test_catalogue_values_and_decisions_agree_with_the_oracle(case):
    _assert_pinned(case.name, yc.judged_oracle(case, ANY_ORDER))


@pytest.mark.parametrize("name", ["harm0_8000", "rand0_8000", "harm2_16384"])
def test_fixture_utterances_agree_with_the_oracle(name, gold):
    kind, n = name.split("_")[0], int(name.split("_")[1])
    wav = synthetic.harm_batch([int(kind[4:])], n) if kind.startswith("harm") else synthetic.rand_batch(int(kind[4:]), 1, n)
    aux = {}
    final = oy.yaapt_one(wav[0], yc.OPTS, aux=aux)
    assert np.array_equal(final.numpy(), gold.npz("fx_f0.npz")[name][0])       # the oracle run IS the reference's track
    res = yc.judge_oracle(aux, oy.Plan(n, yc.OPTS), ANY_ORDER)
    _assert_pinned(name, res)
    for stage, frames in yc.exempt_frames(res).items():          # the pin is not vacuous: nearly every frame is decided
        assert len(frames) <= 0.1 * aux["energy"].numel(), (stage, frames)


def test_raising_cases_have_no_certain_candidate():
    """where the reference raises, the float64 peak lists agree that no frame above the threshold has a candidate"""
    for case in yc.raising():
        aux, _, raised = yc.oracle_run(case)
        assert raised == case.raises
        plan = oy.Plan(case.n, yc.OPTS)
        r = r64.judge_cand(aux["filt2"].numpy(), aux["vuv"].numpy(), aux["cand_pitch"].numpy(), aux["cand_merit"].numpy(), plan, ANY_ORDER)
        assert not r["wrong"] and r["ratio"] <= 1.0, (case, r)


# ---- the judges bite ---------------------------------------------------------------------------------------------------
def _tone_aux():
    case = yc.by_name("tone_20481")
    return yc.oracle_run(case)[0], oy.Plan(case.n, yc.OPTS)


def test_a_rescaled_energy_fails_its_bound():
    aux, plan = _tone_aux()
    e = aux["energy"].numpy()
    assert r64.judge_vuv(aux["filt"].numpy(), e, aux["vuv"].numpy(), plan, ANY_ORDER)["ratio"] <= 1.0
    assert r64.judge_vuv(aux["filt"].numpy(), e * np.float32(1.001), aux["vuv"].numpy(), plan, ANY_ORDER)["ratio"] > 1.0
    flipped = aux["vuv"].numpy().copy()
    flipped[10] = ~flipped[10]
    assert r64.judge_vuv(aux["filt"].numpy(), e, flipped, plan, ANY_ORDER)["wrong"] == [10]
    assert r64.judge_energy_norm(e * 3.0, e, ANY_ORDER)["ratio"] <= 1.0        # normalisation: scale free
    shifted = e.copy()
    shifted[3] *= np.float32(1.0001)
    assert r64.judge_energy_norm(e, shifted, ANY_ORDER)["ratio"] > 1.0


def test_a_moved_peak_or_merit_fails():
    aux, plan = _tone_aux()
    args = (aux["filt2"].numpy(), aux["vuv"].numpy())
    cp, cm = aux["cand_pitch"].numpy().copy(), aux["cand_merit"].numpy().copy()
    assert not r64.judge_cand(*args, cp, cm, plan, ANY_ORDER)["wrong"]
    f = int(np.flatnonzero(cp[0] > 0)[5])
    cp2 = cp.copy()
    cp2[0, f] += np.float32(plan.delta)                    # the neighbouring bin
    assert [w[0] for w in r64.judge_cand(*args, cp2, cm, plan, ANY_ORDER)["wrong"]] == [f]
    cm2 = cm.copy()
    cm2[0, f] *= np.float32(1.001)
    assert r64.judge_cand(*args, cp, cm2, plan, ANY_ORDER)["ratio"] > 1.0


def test_a_shifted_lag_mean_or_merit_fails():
    aux, plan = _tone_aux()
    x = aux["filt"].numpy()
    means = []
    oy.frame_means(aux["filt"], plan, means=means)
    means = np.array([float(m) for m in means], np.float32)
    sp, pstd = aux["spec_pitch"].numpy(), float(aux["pitch_std"])
    tp, tm = aux["tp1"][0].numpy().copy(), aux["tm1"][0].numpy().copy()
    assert r64.judge_fmean(x, means, plan, ANY_ORDER)["ratio"] <= 1.0
    bad = means.copy()
    bad[7] += np.float32(1e-4)
    assert r64.judge_fmean(x, bad, plan, ANY_ORDER)["ratio"] > 1.0
    ok = r64.judge_nccf(x, means, sp, pstd, tp, tm, plan, ANY_ORDER)
    assert not ok["wrong"] and ok["ratio"] <= 1.0
    k = int(np.flatnonzero(tp > 0)[8])
    lag = int(round(16000.0 / float(tp[k]))) - 1
    tp2 = tp.copy()
    tp2[k] = np.float32(16000.0 / float(lag + 2))          # the next lag
    assert [w[0] for w in r64.judge_nccf(x, means, sp, pstd, tp2, tm, plan, ANY_ORDER)["wrong"]] == [k]
    tm2 = tm.copy()
    tm2[k] *= np.float32(1.001)
    assert r64.judge_nccf(x, means, sp, pstd, tp, tm2, plan, ANY_ORDER)["ratio"] > 1.0
    tm3 = tm.copy()
    tm3[k] = np.nan                                        # a NaN on one side only
    assert r64.judge_nccf(x, means, sp, pstd, tp, tm3, plan, ANY_ORDER)["ratio"] == float("inf")


def test_nan_pitch_std_gives_nan_merits_and_no_candidates():
    aux, _, _ = yc.oracle_run(yc.by_name("burst260_at20220_of20480"))
    assert torch.isnan(aux["pitch_std"])
    assert torch.isnan(aux["tm1"][0]).all() and torch.isnan(aux["tm2"][0]).all()
    assert not aux["tp1"].any() and not aux["tp2"].any()


def test_demeaned_frames_are_the_oracles_bit_for_bit():
    aux, plan = _tone_aux()
    means = []
    frames = oy.frame_means(aux["filt"], plan, means=means).numpy()
    means = np.array([float(m) for m in means], np.float32)
    for k in (0, 1, 17, plan.tda_nframes - 1):
        assert np.array_equal(r64.demeaned_frame(aux["filt"].numpy(), k, means, plan), frames[k])


def test_running_fft_bound_holds_for_a_float32_radix2_fft():
    """the kernels' FFT restated in numpy float32 (bit-reversed input, 13 radix-2 stages, twiddles rounded once from
    float64, each butterfly in float32 component arithmetic): its distance from the float64 transform stays under the
    running bound, which in turn stays far under the closed form 13 (cmul + 1) U sum |x|"""
    n = 1120
    t = np.arange(n) / 16000.0
    rng = np.random.default_rng(5)
    frames = np.stack([sum(0.3 / k * np.sin(2 * np.pi * k * 120.0 * t + p) for k in range(1, 6)) for p in (0.0, 1.0)]
                      + [rng.standard_normal(n), np.ones(n)]).astype(np.float32)
    X, E = r64.fft_running(frames.astype(np.float64), np.zeros(frames.shape), ANY_ORDER, 4097)
    rev = sum(((np.arange(8192) >> b) & 1) << (12 - b) for b in range(13))
    xs = np.zeros((frames.shape[0], 8192), np.float32)
    xs[:, :n] = frames
    re, im = xs[:, rev].copy(), np.zeros_like(xs)
    for s in range(1, 14):
        h = 1 << (s - 1)
        ang = 2 * np.pi * np.arange(h) * (4096 // h) / 8192.0
        wr, wi = np.cos(ang).astype(np.float32), (-np.sin(ang)).astype(np.float32)
        re, im = re.reshape(-1, 8192 // (2 * h), 2, h), im.reshape(-1, 8192 // (2 * h), 2, h)
        ar, ai, br, bi = re[:, :, 0], im[:, :, 0], re[:, :, 1], im[:, :, 1]
        tr, ti = br * wr - bi * wi, br * wi + bi * wr
        re = np.concatenate((ar + tr, ar - tr), axis=2).reshape(-1, 8192)
        im = np.concatenate((ai + ti, ai - ti), axis=2).reshape(-1, 8192)
        assert re.dtype == np.float32
    err = np.abs((re[:, :4097].astype(np.float64) + 1j * im[:, :4097].astype(np.float64)) - X)
    ratio = (err / E).max(1)
    closed = 13 * (ANY_ORDER.cmul + 1) * r64.U * np.abs(frames.astype(np.float64)).sum(1)
    print("float32 radix-2 FFT: error / running bound per frame", ratio, " running / closed bound", (E.max(1) / closed))
    assert (ratio <= 1.0).all() and (ratio > 1e-3).all()
    assert (E.max(1) <= closed * 1.002).all()
