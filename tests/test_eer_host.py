"""Host side of the bootstrap interval of the EER, CPU only: the generator of tests/ref64_eer.py against the published Philox known
answers, satools_amd.asv_eval.empirical_eer / eer_cuts against the definition evaluated threshold by threshold, the argument checks of
ops.eer_bootstrap, the unchanged default of the metric functions, the report lines, and the constant of include/satools_hip_stats.h (the
header, the binding and the bounds table are held together by tests/test_components_host.py).  Everything compared here is integers or the
same float64 division on both sides: equality, no tolerance."""
import json
import os

import numpy as np
import pytest
import torch

import abi_decl
import ref64_eer
from satools_amd import _lib, asv_eval, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKED = [([3, 4, 5], [0, 1, 2], 0.0, None), ([0, 1, 2], [3, 4, 5], 1.0, None), ([0], [0], 1.0, None), ([1], [0], 0.0, None),
          ([0, 0, 1, 1, 2], [0, 1, 1, 2, 2, 2], 0.8, (4, 5))]


# ---- the generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    """the Random123 known-answer vectors of philox4x32-10"""
    h = lambda s: [int(x, 16) for x in s.split()]
    got = ref64_eer.philox4x32_10(np.array(h(counter), dtype=np.uint64), h(key))
    assert [int(x) for x in got] == h(want)


def test_words_follow_the_counter_layout():
    """word j of stream s of replicate r = output word j & 3 at the counter (j >> 2, r, s, 0), key = the two halves of the seed"""
    seed = 0x0123456789ABCDEF
    w = ref64_eer.words(11, 5, 1, seed)
    for j in range(11):
        blk = ref64_eer.philox4x32_10(np.array([j >> 2, 5, 1, 0], dtype=np.uint64), (0x89ABCDEF, 0x01234567))
        assert int(w[j]) == int(blk[j & 3])
    assert not np.array_equal(ref64_eer.words(8, 5, 0, seed), w[:8]) and not np.array_equal(ref64_eer.words(8, 6, 1, seed), w[:8])


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 2 ** 20, 2 ** 32 - 1])
def test_draws_are_indices_and_the_word_stream_ignores_the_tail(n):
    count = min(n, 1 << 16)
    d = ref64_eer.draws(n, 3, 0, 7, count=count)
    assert d.shape == (count,) and d.min() >= 0 and d.max() < n
    w = ref64_eer.words(n, 3, 0, 7, count=count)
    assert np.array_equal(d, (w.astype(object) * n) >> 32)                      # (Python integers: no width to overflow)
    assert (0xFFFFFFFF * n) >> 32 == n - 1                                        # the largest word gives the last index
    if n < 2 ** 20:                                                               # the same words whatever the remainder of n mod 4
        for more in (1, 2, 3, 4):
            assert np.array_equal(ref64_eer.words(n + more, 3, 0, 7)[:n], w)
        assert np.array_equal(ref64_eer.words(4 * n, 3, 0, 7)[:4 * (n // 4)], ref64_eer.words(4 * (n // 4) + 4, 3, 0, 7)[:4 * (n // 4)])
    if n >= 2 ** 20:
        assert len(np.unique(d)) > 0.9 * count                                    # (spread over the whole range, not a corner of it)


# ---- the statistic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tar, non, eer, counts", WORKED)
def test_empirical_eer_worked_cases(tar, non, eer, counts):
    got = asv_eval.empirical_eer(tar, non)
    assert got == ref64_eer.brute_eer(tar, non) and got[0] == eer
    if counts:
        assert got[1:] == counts


def _small_lists(n=200):
    g = np.random.default_rng(1)
    for _ in range(n):
        yield g.integers(0, 3, g.integers(1, 10)).astype(np.float64), g.integers(0, 3, g.integers(1, 10)).astype(np.float64)


def test_empirical_eer_equals_the_definition_on_small_lists_with_heavy_ties():
    seen = set()
    for tar, non in _small_lists():
        got = asv_eval.empirical_eer(tar, non)
        assert got == ref64_eer.brute_eer(tar, non), (tar, non)
        ts, ns = np.sort(tar), np.sort(non)
        assert got[1:] == ref64_eer.eer_counts(ts, ns, np.arange(len(ts)), np.arange(len(ns)))      # identity draws: the sets themselves
        assert isinstance(got[1], int) and isinstance(got[2], int)
        seen.add(got[0])
    assert {0.0, 1.0} <= seen and len(seen) > 10


def test_histogram_restatement_equals_the_definition_under_resampling():
    """tests/ref64_eer.py against itself: eer_counts (histogram, prefix sum) and brute_eer (weights) on resampled small lists"""
    g = np.random.default_rng(2)
    for tar, non in _small_lists(100):
        ts, ns = np.sort(tar), np.sort(non)
        it, inn = g.integers(0, len(ts), len(ts)), g.integers(0, len(ns), len(ns))
        w = (np.bincount(it, minlength=len(ts)), np.bincount(inn, minlength=len(ns)))
        assert ref64_eer.eer_counts(ts, ns, it, inn) == ref64_eer.brute_eer(ts, ns, w)[1:]


def test_eer_cuts():
    for tar, non in list(_small_lists(50)) + [(np.random.default_rng(3).normal(1, 1, 500), np.random.default_rng(4).normal(-1, 1, 700))]:
        ts, ns = np.sort(tar), np.sort(non)
        ct, cn = asv_eval.eer_cuts(ts, ns)
        v = np.unique(np.concatenate([ts, ns]))
        K = len(v)
        assert ct.dtype == cn.dtype == np.int32 and ct.shape == cn.shape == (K + 1,)
        assert np.all(np.diff(ct) >= 0) and np.all(np.diff(cn) >= 0)
        assert ct[0] == cn[0] == 0 and ct[K] == len(ts) and cn[K] == len(ns)
        assert ct[:K].tolist() == [int((ts < x).sum()) for x in v] and cn[:K].tolist() == [int((ns < x).sum()) for x in v]
    with pytest.raises(ValueError):
        asv_eval.eer_cuts([2.0, 1.0], [0.0])
    with pytest.raises(ValueError):
        asv_eval.eer_cuts([1.0, float("nan")], [0.0])


def test_empirical_eer_is_never_below_the_rocch_eer():
    g = np.random.default_rng(5)
    for n in (30, 300):
        tar, non = g.normal(1, 1, n), g.normal(-1, 1, 2 * n)
        assert asv_eval.empirical_eer(tar, non)[0] >= asv_eval.calibrate(tar, non)["eer"] - 1e-12


# ---- ops.eer_bootstrap: refusals on the host, before any device call -------------------------------------------------------
def test_ops_eer_bootstrap_checks_its_arguments_before_any_device_call(monkeypatch):
    def no_device_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "lib", no_device_call)
    ct, cn = asv_eval.eer_cuts([0.0, 1.0, 2.0], [0.5, 1.0])                       # K = 4
    ok = dict(n_tar=3, n_non=2, m=4)
    bad = ct.copy()
    bad[1], bad[2] = 2, 1
    cases = {
        "non-monotone": ((bad, cn), ok), "wrong end value": ((ct, np.append(cn[:-1], 3).astype(np.int32)), ok),
        "m = 0": ((ct, cn), dict(ok, m=0)), "n_tar = 0": ((ct, cn), dict(ok, n_tar=0)), "different lengths": ((ct, cn[1:]), ok),
        "not integers": ((ct.astype(np.float64), cn), ok), "no table starts at 0": ((ct + np.int32([1, 0, 0, 0, 0]), np.maximum(cn, 1)), ok),
        "negative first replicate": ((ct, cn), dict(ok, first_replicate=-1)), "replicates past 2^31": ((ct, cn), dict(ok, first_replicate=2 ** 31 - 4)),
        "a side above the maximum": ((np.int32([0, 2 ** 20 + 1]), np.int32([0, 1])), dict(n_tar=2 ** 20 + 1, n_non=1, m=1)),
        "seed of more than 64 bits": ((ct, cn), dict(ok, seed=2 ** 64)),
        "a host device": ((ct, cn), dict(ok, device="cpu")),
    }
    for what, (tables, kw) in cases.items():
        with pytest.raises(_lib.SatError):
            ops.eer_bootstrap(*tables, **kw)
            pytest.fail(what)
    if not torch.cuda.is_available():                                             # no device: refused like every other op, no CPU fallback
        with pytest.raises(_lib.SatError, match="no CPU fallback"):
            ops.eer_bootstrap(ct, cn, **ok)
        with pytest.raises(_lib.SatError, match="no CPU fallback"):
            asv_eval.eer_interval([0.0, 1.0, 2.0], [0.5, 1.0], m=4)


def test_eer_interval_takes_the_percentiles_at_exactly_the_nominal_points(monkeypatch):
    """eer_interval with the restatement standing in for the device: the interval of ci = 0.95 is np.percentile(replicates, [2.5, 97.5]) to
    the last bit (50 * (1 - 0.95) is 2.500000000000002 in float64: a percentile taken there differs by an ulp), likewise 0.9 and 0.5"""
    g = np.random.default_rng(2024)
    tar, non = g.normal(1, 1, 300), g.normal(-1, 1, 200)

    def stand_in(ct, cn, n_tar, n_non, m, seed=0, first_replicate=0, device=None):
        assert (ct.tolist(), cn.tolist()) == tuple(x.tolist() for x in asv_eval.eer_cuts(np.sort(tar), np.sort(non)))
        miss, fa = ref64_eer.replicates(np.sort(tar), np.sort(non), first_replicate, m, seed)
        return torch.from_numpy(miss).to(torch.int32), torch.from_numpy(fa).to(torch.int32)
    monkeypatch.setattr(ops, "eer_bootstrap", stand_in)
    miss, fa = ref64_eer.replicates(np.sort(tar), np.sort(non), 0, 400, 5)
    w = np.minimum(miss.astype(np.float64) / 300, fa.astype(np.float64) / 200)
    for ci, points in ((0.95, [2.5, 97.5]), (0.9, [5.0, 95.0]), (0.5, [25.0, 75.0])):
        eer, lower, upper, reps = asv_eval.eer_interval(tar, non, m=400, ci=ci, seed=5)
        assert reps.tobytes() == w.tobytes() and eer == asv_eval.empirical_eer(tar, non)[0]
        assert [lower, upper] == [float(x) for x in np.percentile(w, points)] and 0.0 <= lower <= upper <= 1.0


# ---- the metric functions: nothing changes without the option --------------------------------------------------------------
def _same(a, b):
    assert json.dumps({k: v for k, v in a.items() if k != "score"}, sort_keys=True) == json.dumps({k: v for k, v in b.items() if k != "score"}, sort_keys=True)
    for x, y in zip(a["score"], b["score"]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_metrics_without_the_option_are_what_they_were(tmp_path, monkeypatch):
    fx = np.load(os.path.join(ROOT, "tests", "golden", "fx_asv_eval.npz"))
    for case in ("separated", "tied", "few_mated"):
        a = asv_eval.score_metrics(fx[case + "/mated"], fx[case + "/non"])
        b = asv_eval.score_metrics(fx[case + "/mated"], fx[case + "/non"], eer_ci=None)
        _same(dict(a[0], score=a[1:]), dict(b[0], score=b[1:]))
    case = "c50_t300"
    ie, it, target = fx[case + "/idx_e"], fx[case + "/idx_t"], fx[case + "/target"]
    trials = tmp_path / "trials"
    trials.write_text("".join(f"s{a} t{b} {'target' if t else 'nontarget'}\n" for a, b, t in zip(ie, it, target)))
    # (the scoring needs the device: the recorded scores of the fixture stand in for it; the metrics are host work)
    monkeypatch.setattr(asv_eval, "score_trials", lambda *a, **k: (fx[case + "/scores"].astype(np.float32), fx[case + "/asnorm"].astype(np.float32)))
    a = asv_eval.compute_metrics({}, {}, {}, str(trials), str(tmp_path / "a"), cohort=object())
    b = asv_eval.compute_metrics({}, {}, {}, str(trials), str(tmp_path / "b"), cohort=object(), eer_ci=None)
    _same(a, b)
    _same(dict(a["asnorm"], score=()), dict(b["asnorm"], score=()))
    assert open(tmp_path / "a" / "scores").read() == open(tmp_path / "b" / "scores").read()
    try:
        import feerci  # noqa: F401
    except ImportError:
        assert a["eer_lower"] is None and a["eer_upper"] is None and a["asnorm"]["eer_lower"] is None
        s = fx[case + "/scores"].astype(np.float32).astype(np.float64)
        assert a["eer"] == 100 * asv_eval.calibrate(s[target], s[~target])["eer"]      # still the ROCCH-EER


def test_score_metrics_with_the_option_takes_all_three_from_the_interval(monkeypatch):
    """the plumbing, without a device: eer_interval is handed the calibrated LLRs and the options, its three results land x 100"""
    try:
        import feerci  # noqa: F401
        pytest.skip("feerci is importable and wins")
    except ImportError:
        pass
    fx = np.load(os.path.join(ROOT, "tests", "golden", "fx_asv_eval.npz"))
    seen = {}

    def fake(tar, non, **kw):
        seen.update(kw, tar=tar, non=non)
        return 0.25, 0.125, 0.5, np.zeros(kw["m"])
    monkeypatch.setattr(asv_eval, "eer_interval", fake)
    plain, tar, non = asv_eval.score_metrics(fx["tied/mated"], fx["tied/non"])
    m, tar2, non2 = asv_eval.score_metrics(fx["tied/mated"], fx["tied/non"], eer_ci=dict(m=64, ci=0.9, seed=3))
    assert (m["eer"], m["eer_lower"], m["eer_upper"]) == (25.0, 12.5, 50.0)
    assert set(m) == set(plain) and all(m[k] == plain[k] for k in ("linkability", "min_cllr", "eer_threshold"))
    assert (seen["m"], seen["ci"], seen["seed"]) == (64, 0.9, 3) and seen["tar"] is tar2 and seen["non"] is non2
    assert tar.tobytes() == tar2.tobytes() and non.tobytes() == non2.tobytes()


def test_report_lines_with_and_without_an_interval():
    m = {"eer": 12.34567, "eer_lower": 11.0, "eer_upper": 13.5004, "min_cllr": 0.45678, "linkability": 0.30049, "eer_threshold": 0.1,
         "asnorm": {"eer": 9.87654, "eer_lower": None, "eer_upper": None, "min_cllr": 0.4, "linkability": 0.25, "eer_threshold": 0.0}}
    assert asv_eval.report_lines(m) == [" %EER: 12.346 ± 1.25, Min Cllr: 0.457, linkability: 0.3", " %EER: 9.877, Min Cllr: 0.4, linkability: 0.25"]
    m["asnorm"] = {k: None for k in m["asnorm"]}                                  # no cohort: one line
    assert asv_eval.report_lines(m) == [" %EER: 12.346 ± 1.25, Min Cllr: 0.457, linkability: 0.3"]


def test_command_line_has_the_new_options(capsys):
    with pytest.raises(SystemExit):
        asv_eval.main(["--help"])
    text = capsys.readouterr().out
    assert "--eer-ci M" in text and "--eer-ci-seed S" in text and "--report" in text


# ---- what is particular to this component (tests/test_components_host.py holds header, binding, library, build and bounds table together) ----
def test_stats_header_maximum_is_the_one_ops_checks():
    maximum = int(abi_decl.define("satools_hip_stats.h", "SAT_EER_BOOTSTRAP_MAX_SIDE"))
    assert maximum >= 2 ** 20 and maximum == ops.EER_BOOTSTRAP_MAX_SIDE
    assert callable(ops.eer_bootstrap) and callable(asv_eval.eer_interval)
