"""Host side of the ASV evaluation, CPU only: the C-ABI surface of csrc/asv_score.hip, the float64 metrics of
satools_amd.asv_eval against the reference's recorded results (tests/golden/fx_asv_eval.npz, written by
tests/golden/make_asv_eval_fixtures.py from the reference's own scoring functions), and tests/ref64_asv.py against the
reference's recorded asnorm.

TOLERANCE of the metric comparisons: both sides are float64 and evaluate the same formulae in different orders (histogram
densities, the PAV block means as sums over counts here and as running averages there, means of n logarithms), so they may differ
by the roundings of n-term float64 sums: n 2^-52 times the magnitude of the quantity, n = the number of scores.  A quantity whose
recorded value is exactly 0 (the EER and min Cllr of separated sets, the linkability of one bin) has no magnitude to scale by: there
the absolute tolerance n 2^-52 holds.  Infinite calibrated LLRs must be infinite on both sides."""
import os
import re

import numpy as np
import pytest
import torch

import ref64_asv
from ref64 import U, reduction_terms
from satools_amd import _lib, asv_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sat_cohort_topk_stats_f32", "sat_trial_scores_f32", "sat_segment_mean_l2norm_f32")
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "fx_asv_eval.npz"))


def test_new_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "satools_hip.h")).read()
    assert int(re.search(r"#define SAT_ABI_VERSION (\d+)", header).group(1)) == 8       # additive: no new ABI number
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.symbols("core")
    from satools_amd import ops
    for fn in ("cohort_topk_stats", "trial_scores", "segment_mean_l2norm"):
        assert callable(getattr(ops, fn))


def test_a_library_without_a_bound_symbol_is_reported_with_the_build_command(monkeypatch):
    """what a library built before the ASV entries existed looks like to the binding: a name of the table that dlsym cannot find"""
    import ctypes as C
    monkeypatch.setitem(_lib.COMPONENTS["core"], "sat_entry_of_a_newer_tree_f32", (C.c_int, []))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.SatError, match=r"does not export sat_entry_of_a_newer_tree_f32.*build\.py"):
        _lib.lib()


def test_ops_refuse_host_tensors_and_bad_index_lists():
    from satools_amd import ops
    with pytest.raises(_lib.SatError):
        ops.cohort_topk_stats(torch.zeros(2, 4), torch.zeros(3, 4))
    with pytest.raises(_lib.SatError):
        ops.trial_scores(torch.zeros(2, 4), torch.zeros(3, 4), [0], [0])
    with pytest.raises(_lib.SatError):
        ops._host_i32([0.5, 1.0], "x")
    with pytest.raises(_lib.SatError):
        ops._host_i32([], "x")


def _close(name, got, want, n, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf]), (name, "infinite entries differ")
    mag = np.abs(want[~inf]) if scale is None else np.broadcast_to(np.float64(scale), want[~inf].shape)
    tol = n * EPS * np.where(mag == 0, 1.0, mag)
    err = np.abs(got[~inf] - want[~inf])
    r = float((err / tol).max()) if err.size else 0.0
    print(f"{name}: max error {float(err.max()) if err.size else 0.0:.3e}, error / tolerance {r:.4f}")
    assert r <= 1.0, (name, r)


def _score_sets(fx):
    out = []
    for case in ("separated", "tied", "few_mated"):
        out.append((case, fx[case + "/mated"], fx[case + "/non"], case + "/"))
    for case in ("c50_t300", "c1000_t5000"):
        t = fx[case + "/target"]
        out.append((case + "-raw", fx[case + "/scores"][t], fx[case + "/scores"][~t], case + "/raw/"))
        a = fx[case + "/asnorm"].astype(np.float64)
        out.append((case + "-asnorm", a[t], a[~t], case + "/as/"))
    return out


def test_host_metrics_match_the_reference(fx):
    seen = set()
    for name, mated, non, key in _score_sets(fx):
        n = len(mated) + len(non)
        d_sys = asv_eval.linkability(mated, non)[0]
        cmin, eer, tar, nontar = asv_eval.min_cllr(mated, non)
        _close(name + " linkability", d_sys, fx[key + "linkability"], n)
        _close(name + " min_cllr", cmin, fx[key + "min_cllr"], n)
        _close(name + " rocch eer", eer, fx[key + "eer"], n)
        _close(name + " target llrs", tar, fx[key + "tar_llrs"], n)
        _close(name + " non-target llrs", nontar, fx[key + "non_llrs"], n)
        seen.add(name)
    assert len(seen) == 7


def test_fixture_cases_are_what_they_claim(fx):
    """well separated, heavily tied, one linkability bin, overlapping vector cases with k < 200 and k = 200"""
    assert fx["separated/mated"].min() > fx["separated/non"].max() and float(fx["separated/eer"]) == 0.0
    both = np.concatenate([fx["tied/mated"], fx["tied/non"]])
    assert len(np.unique(both)) < len(both) / 20 and len(np.intersect1d(fx["tied/mated"], fx["tied/non"])) > 5
    assert 10 <= len(fx["few_mated/mated"]) < 20
    assert asv_eval.linkability(fx["few_mated/mated"], fx["few_mated/non"])[1].shape == (1,)       # the reference's nBins rule: one bin
    assert float(fx["few_mated/linkability"]) == 0.0
    for case, C, M in (("c50_t300", 50, 300), ("c1000_t5000", 1000, 5000)):
        assert fx[case + "/cohort_f16"].shape == (C, 192) and fx[case + "/scores"].shape == (M,)
        t = fx[case + "/target"]
        s = fx[case + "/scores"]
        assert s[t].mean() > s[~t].mean() and s[t].min() < s[~t].max()             # mated above non-mated, overlapping


def test_score_metrics_has_the_references_keys_without_feerci(fx):
    m, tar, non = asv_eval.score_metrics(fx["tied/mated"], fx["tied/non"])
    assert set(m) == {"linkability", "eer", "eer_lower", "eer_upper", "min_cllr", "eer_threshold"}
    try:
        import feerci  # noqa: F401
    except ImportError:
        assert m["eer_lower"] is None and m["eer_upper"] is None
        _close("eer x 100", m["eer"], 100 * fx["tied/eer"], 1700)
        assert np.isfinite(m["eer_threshold"])
    assert len(tar) == 200 and len(non) == 1500


def test_pav_is_the_isotonic_fit():
    g = np.random.default_rng(0)
    for n in (1, 2, 7, 200):
        y = g.integers(0, 2, n).astype(np.float64)
        fit, w, h = asv_eval.pav(y)
        assert np.all(np.diff(fit) >= 0) and w.sum() == n and np.all(np.diff(h) > 0)
        assert np.allclose(np.repeat(h, w), fit)
        pos = np.concatenate([[0], np.cumsum(w)])                          # every block is the mean of its points
        for a, b, hv in zip(pos[:-1], pos[1:], h):
            assert abs(y[a:b].mean() - hv) < 1e-15


@pytest.mark.parametrize("case", ("c50_t300", "c1000_t5000"))
def test_ref64_asv_in_float32_reproduces_the_references_asnorm(fx, case):
    """pins that tests/ref64_asv.py restates the reference: evaluated in float32 (the reference's precision) from the reference's
    recorded cosine scores, it meets the recorded asnorm within the bound the device is held to — and so does the float64 evaluation."""
    enroll, test = torch.from_numpy(fx[case + "/enroll"]), torch.from_numpy(fx[case + "/test"])
    cohort = torch.from_numpy(fx[case + "/cohort_f16"].astype(np.float32))
    ie, it = fx[case + "/idx_e"], fx[case + "/idx_t"]
    C, D = cohort.shape
    k = min(200, C)
    want = torch.from_numpy(fx[case + "/asnorm"]).double()
    s32 = torch.from_numpy(fx[case + "/scores"]).float()                  # the reference feeds asnorm its scores as float32

    def asnorm(scores):
        me, se, ae = ref64_asv.cohort_topk_stats(enroll, cohort, k)
        mt, st, at = ref64_asv.cohort_topk_stats(test, cohort, k)
        s = ref64_asv._d(scores)
        return 0.5 * ((s - me[ie]) / se[ie] + (s - mt[it]) / st[it]), (me, se, mt, st), (ae, at)

    exact, stats, (ae, at) = asnorm(s32)
    dme, _ = ref64_asv.topk_mean_bound(ae, C, D, k)
    dmt, _ = ref64_asv.topk_mean_bound(at, C, D, k)
    dse = ref64_asv.topk_std_bound(ae, stats[1], C, D, k)
    dst = ref64_asv.topk_std_bound(at, stats[3], C, D, k)
    bound = ref64_asv.asnorm_bound(s32.double(), torch.zeros(()), stats, (dme, dse, dmt, dst), ie, it)
    r64 = float(((exact - want).abs() / bound).max())
    with ref64_asv.in_float32():
        got32 = asnorm(s32)[0].double()
    r32 = float(((got32 - want).abs() / bound).max())
    print(f"{case}: recorded asnorm vs ref64_asv in float64: error / bound {r64:.4f}; in float32: {r32:.4f}; "
          f"largest bound {float(bound.max()):.3e}")
    assert r64 <= 1.0 and r32 <= 1.0


def test_ref64_asv_trial_scores_match_the_recorded_cosine(fx):
    for case in ("c50_t300", "c1000_t5000"):
        s, _, aux = ref64_asv.trial_scores(fx[case + "/enroll"], fx[case + "/test"], fx[case + "/idx_e"], fx[case + "/idx_t"])
        bound = ref64_asv.score_bound(s, aux, 192)                         # the reference's own float32 / float64 evaluation
        r = float(((s - torch.from_numpy(fx[case + "/scores"])).abs() / bound).max())
        print(f"{case}: recorded cosine vs ref64_asv: error / bound {r:.4f}")
        assert r <= 1.0


def test_read_trials_and_synthetic_xvector_spec(tmp_path):
    p = tmp_path / "trials"
    p.write_text("spk1 utt1 target\nspk1 utt2 nontarget\n\n")
    assert asv_eval.read_trials(str(p)) == (["spk1", "spk1"], ["utt1", "utt2"], ["target", "nontarget"])
    import satools_amd
    m = satools_amd.load_model("synthetic:xvector?seed=1&speakers=7")
    assert tuple(m.after_speaker_embedding.weight.shape) == (7, 192)
    assert reduction_terms(192) == 11 and U == 2.0 ** -24
