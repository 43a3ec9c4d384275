"""The ASV scoring kernels (csrc/asv_score.hip) and the evaluation built on them (satools_amd.asv_eval), each against the float64
restatement in tests/ref64_asv.py with DERIVED bounds (the error model is in that file's docstring; U = 2^-24, k(n) of
tests/ref64.py).  Needs a real MI355X: run with `-m gpu` (`-s` prints the largest observed error / bound per kernel; a ratio above
1 fails; SAT_ASV_RATIOS names a file to write the table to).

No case is left out for near-ties at the k-th place: the bound on the top-k statistics holds whatever the ties (sorted lists of two
score sets within E of each other are within E elementwise).  Rows whose deviation is 0 (k identical scores) check the statistics
only, their s-norm divides by zero on both sides.

MEASURED on an MI355X (profiles/asv_score_error_ratios.txt), largest error / bound per kernel:
  cohort_topk_stats mean 0.13 (randn, N 1027, C 5994, D 4, k 1), std 0.06 | exact-integer scores: mean 0.90 (its bound is ONE rounding), std 0.11
  trial_scores cosine 0.14, s-norm 0.02 | segment_mean_l2norm 0.18; single-utterance rows equal bit for bit
  compute_metrics against the reference's recorded scores 0.08, s-norm scores 0.03 | test_metrics scores on the toy directory 0.04.
(The deviation and s-norm ratios were recorded while topk_std_bound still carried E sqrt(k / (k - 1)) twice; against the present bound
they are at most twice these figures.)"""
import json
import math
import os

import numpy as np
import pytest
import torch

import ref64_asv
from ref64 import U, reduction_terms

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden")

N_GRID = (1, 3, 4, 5, 1027)
C_GRID = (1, 2, 63, 64, 65, 199, 200, 201, 1000, 5994, 8192)
D_GRID = (4, 192, 256, 512)

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    lines = [f"{k:28s} {r:8.4f}   at {case}" for k, (r, case) in sorted(_RATIOS.items())]
    print("\nlargest observed error / derived bound, per kernel:\n" + "\n".join(lines))
    path = os.environ.get("SAT_ASV_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_asv_score.py: largest observed error / derived bound, per kernel (a ratio above 1 fails)\n")
            f.write("\n".join(lines) + "\n")


def _ops():
    import satools_amd  # noqa: F401
    from satools_amd import ops
    return ops


def _sat_error():
    import satools_amd  # noqa: F401
    from satools_amd import _lib
    return _lib.SatError


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _check(kernel, case, got, want, bound, quiet=False):
    got = torch.as_tensor(got).detach().cpu().double()
    want, bound = torch.as_tensor(want).double(), torch.as_tensor(bound, dtype=torch.float64)
    assert got.shape == want.shape, (kernel, case, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), (kernel, case, "non-finite output")
    err = (got - want).abs()
    bound = bound.expand_as(err)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = float(ratio.max()) if ratio.numel() else 0.0
    if not quiet:
        print(f"{kernel} [{case}]: max error {float(err.max()):.3e}, max error / bound {r:.4f}")
    if r > _RATIOS.get(kernel, (-1.0, ""))[0]:
        _RATIOS[kernel] = (r, case)
    assert r <= 1.0, (kernel, case, r, float(err.max()))
    return r


def _unit(x):
    return x / x.norm(dim=1, keepdim=True).clamp(min=1e-30)


def _vectors(kind, N, C, D, g):
    if kind == "unit":                   # x-vectors against class centres: the top scores sit in a narrow band
        centres = torch.randn(8, D, generator=g)
        x = _unit(centres[torch.arange(N) % 8] + 0.7 * torch.randn(N, D, generator=g))
        c = _unit(centres[torch.arange(C) % 8] + 1.5 * torch.randn(C, D, generator=g))
        return x, c
    return 3.0 * torch.randn(N, D, generator=g), torch.randn(C, D, generator=g) + 0.25


def _still_works():
    x = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0]])
    c = torch.tensor([[1.0, 1.0, 0.0, 0.0], [3.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0]])
    m, s = _ops().cohort_topk_stats(x.to(DEV), c.to(DEV), 2)
    torch.cuda.synchronize()
    assert torch.equal(m.cpu(), torch.tensor([2.0, 1.0])) and torch.equal(s.cpu(), torch.tensor([2.0, 2.0]).sqrt())


# ---- cohort_topk_stats ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", D_GRID, ids=lambda d: f"D{d}")
@pytest.mark.parametrize("C", C_GRID, ids=lambda c: f"C{c}")
def test_cohort_topk_stats(C, D):
    ops = _ops()
    for N in N_GRID:
        for k in sorted({min(200, C), 1, C}):
            for kind in ("unit", "randn") if N in (5, 1027) else ("unit",):
                x, c = _vectors(kind, N, C, D, _gen(1, N, C, D, k, len(kind)))
                mean, std = ops.cohort_topk_stats(x.to(DEV), c.to(DEV), k)
                assert mean.shape == std.shape == (N,)
                wm, ws, aux = ref64_asv.cohort_topk_stats(x, c, k)
                bm, _E = ref64_asv.topk_mean_bound(aux, C, D, k)
                case = f"{kind}-N{N}-C{C}-D{D}-k{k}"
                _check("cohort_topk_stats mean", case, mean, wm, bm, quiet=True)
                if k == 1:
                    assert bool(torch.isnan(std).all()), case               # torch.std of one value
                else:
                    _check("cohort_topk_stats std", case, std, ws, ref64_asv.topk_std_bound(aux, ws, C, D, k), quiet=True)


def test_cohort_topk_stats_exact_scores_with_ties_across_the_kth_place():
    """small integers: every dot product and every partial sum of the top k is an integer below 2^24, exact in float32 in any order, so
    the mean carries ONE rounding (the division) and the copies of duplicated cohort rows on either side of the k-th place must not
    matter; the deviation carries the arithmetic of its own pass only (E = 0)"""
    ops = _ops()
    g = _gen(2)
    D, C, N = 16, 300, 37
    base = torch.randint(-3, 4, (40, D), generator=g).float()
    c = base[torch.randint(0, 40, (C,), generator=g)]                        # 40 distinct rows, ~7 copies each
    x = torch.randint(-3, 4, (N, D), generator=g).float()
    for k in (200, 7, 150, 299, 300):
        wm, ws, aux = ref64_asv.cohort_topk_stats(x, c, k)
        top = aux["topk"]
        straddle = (x.double() @ c.double().t() == top[:, -1:]).sum(1) > (top == top[:, -1:]).sum(1)
        assert k == C or bool(straddle.any()), "no row has copies of the k-th score outside the top k"
        mean, std = ops.cohort_topk_stats(x.to(DEV), c.to(DEV), k)
        _check("cohort_topk_stats exact mean", f"k{k}", mean, wm, U * wm.abs())
        aux0 = dict(aux, S=torch.zeros_like(aux["S"]), A=torch.zeros_like(aux["A"]))
        bs = ref64_asv.topk_std_bound(aux0, ws, C, D, k) + math.sqrt(k / (k - 1.0)) * U * wm.abs()
        _check("cohort_topk_stats exact std", f"k{k}", std, ws, bs)


def test_cohort_topk_stats_refuses_what_it_cannot_hold():
    ops, SatError = _ops(), _sat_error()
    z = lambda n, d: torch.zeros(n, d, device=DEV)
    for x, c, k, what in ((z(2, 4), z(8193, 4), 200, "C = 8193"), (z(2, 6), z(10, 6), 5, "D = 6"), (z(2, 516), z(10, 516), 5, "D = 516"),
                          (z(2, 8), z(10, 8), 11, "k = 11"), (z(2, 8), z(10, 8), 0, "k = 0")):
        with pytest.raises(SatError, match=r"failed \(-1\).*" + what):
            ops.cohort_topk_stats(x, c, k)
    with pytest.raises(SatError):
        ops.cohort_topk_stats(z(2, 8), z(10, 4), 3)
    _still_works()


# ---- trial_scores ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (4, 7, 65, 192, 256, 512), ids=lambda d: f"D{d}")
@pytest.mark.parametrize("M", (1, 3, 4, 5, 1027), ids=lambda m: f"M{m}")
def test_trial_scores_cosine(M, D):
    ops = _ops()
    g = _gen(3, M, D)
    E, T = 5, 37
    enroll, test = torch.randn(E, D, generator=g), _unit(torch.randn(T, D, generator=g)) * 3.0
    ie, it = torch.randint(0, E, (M,), generator=g).numpy(), torch.randint(0, T, (M,), generator=g).numpy()
    got = ops.trial_scores(enroll.to(DEV), test.to(DEV), ie, it)
    want, _, aux = ref64_asv.trial_scores(enroll, test, ie, it)
    _check("trial_scores cosine", f"M{M}-D{D}", got, want, ref64_asv.score_bound(want, aux, D))


@pytest.mark.parametrize("C", (1, 50, 200, 1000, 5994), ids=lambda c: f"C{c}")
def test_trial_scores_asnorm_from_device_statistics(C):
    """the whole chain: statistics per enrolment and per test row from cohort_topk_stats, gathered per trial by trial_scores;
    first-order propagation per element: (ds + dmu) / sd + |s - mu| dsd / sd^2, halved and summed over the two sides"""
    ops = _ops()
    D, E, T, M = 192, 9, 41, 700
    g = _gen(4, C)
    k = min(200, C)
    enroll, cohort = _vectors("unit", E, C, D, g)
    test = _unit(enroll[torch.arange(T) % E] + 0.08 * torch.randn(T, D, generator=g) * math.sqrt(D) * 0.2)
    ie, it = torch.randint(0, E, (M,), generator=g).numpy(), torch.randint(0, T, (M,), generator=g).numpy()
    de, dt, dc = enroll.to(DEV), test.to(DEV), cohort.to(DEV)
    st_e, st_t = ops.cohort_topk_stats(de, dc, k), ops.cohort_topk_stats(dt, dc, k)
    score, score_as = ops.trial_scores(de, dt, ie, it, (st_e[0], st_e[1], st_t[0], st_t[1]))
    me, se, ae = ref64_asv.cohort_topk_stats(enroll, cohort, k)
    mt, st, at = ref64_asv.cohort_topk_stats(test, cohort, k)
    s64, as64, aux = ref64_asv.trial_scores(enroll, test, ie, it, (me, se, mt, st))
    ds = ref64_asv.score_bound(s64, aux, D)
    _check("trial_scores cosine", f"asnorm-C{C}", score, s64, ds)
    dme, dmt = ref64_asv.topk_mean_bound(ae, C, D, k)[0], ref64_asv.topk_mean_bound(at, C, D, k)[0]
    _check("cohort_topk_stats mean", f"asnorm-C{C}", torch.cat([st_e[0], st_t[0]]), torch.cat([me, mt]), torch.cat([dme, dmt]))
    if k == 1:
        assert bool(torch.isnan(score_as).all())                           # std of one value is NaN, as in the reference
        return
    dse, dst = ref64_asv.topk_std_bound(ae, se, C, D, k), ref64_asv.topk_std_bound(at, st, C, D, k)
    _check("cohort_topk_stats std", f"asnorm-C{C}", torch.cat([st_e[1], st_t[1]]), torch.cat([se, st]), torch.cat([dse, dst]))
    live = torch.as_tensor((se[ie] > 0) & (st[it] > 0))                    # rows whose deviation is 0 check the statistics only
    assert bool(live.any())
    bound = ref64_asv.asnorm_bound(s64, ds, (me, se, mt, st), (dme, dse, dmt, dst), ie, it)
    _check("trial_scores asnorm", f"C{C}", score_as.cpu()[live], as64[live], bound[live])


def test_trial_scores_refuses_an_index_outside_its_table():
    ops, SatError = _ops(), _sat_error()
    e, t = torch.randn(5, 8, device=DEV), torch.randn(7, 8, device=DEV)
    for ie, it, what in (([0, 5], [0, 0], "enrolment row 5 of 5"), ([0, 1], [7, 0], "test row 7 of 7"), ([-1, 1], [0, 0], "enrolment row -1")):
        with pytest.raises(SatError, match=r"failed \(-1\).*" + what):
            ops.trial_scores(e, t, ie, it)
    with pytest.raises(SatError):
        ops.trial_scores(e, t, [0, 1], [0])
    _still_works()
    got = ops.trial_scores(e, t, [4], [6]).cpu()
    want = ref64_asv.trial_scores(e.cpu(), t.cpu(), [4], [6])[0]
    assert abs(float(got[0]) - float(want[0])) < 1e-5


# ---- segment_mean_l2norm -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (4, 65, 192, 512), ids=lambda d: f"D{d}")
def test_segment_mean_l2norm(D):
    ops = _ops()
    g = _gen(5, D)
    sizes = [1, 3, 1, 2, 7, 1, 64, 1, 5]
    Ux = sum(sizes)
    x = _unit(torch.randn(Ux, D, generator=g) + 0.5)
    order = torch.randperm(Ux, generator=g).numpy()
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    got = ops.segment_mean_l2norm(x.to(DEV), order, offsets).cpu()
    want, aux = ref64_asv.segment_mean_l2norm(x, order, offsets)
    for s, n in enumerate(sizes):
        if n == 1:
            assert torch.equal(got[s], x[order[offsets[s]]]), s              # one utterance: the row itself, bit for bit
    _check("segment_mean_l2norm", f"D{D}", got, want, ref64_asv.segment_bound(want, aux, D))
    SatError = _sat_error()
    with pytest.raises(SatError, match=r"failed \(-1\)"):
        ops.segment_mean_l2norm(x.to(DEV), np.where(order == 3, Ux, order), offsets)
    with pytest.raises(SatError, match=r"failed \(-1\)"):
        ops.segment_mean_l2norm(x.to(DEV), order, np.concatenate([[0, 0], np.cumsum(sizes)[1:]]))
    _still_works()


# ---- compute_metrics on the reference's recorded case ----------------------------------------------------------------------
def _fixture_case(fx, case, tmp_path):
    enroll, test = torch.from_numpy(fx[case + "/enroll"]), torch.from_numpy(fx[case + "/test"])
    cohort = torch.from_numpy(fx[case + "/cohort_f16"].astype(np.float32))
    ie, it, target = fx[case + "/idx_e"], fx[case + "/idx_t"], fx[case + "/target"]
    u2e = {f"e{i}": enroll[i] for i in range(len(enroll))}
    u2t = {f"t{j}": test[j] for j in range(len(test))}
    spk2utt = {f"s{i}": [f"e{i}"] for i in range(len(enroll))}               # the recorded rows ARE the per-speaker vectors: copied as they are
    trials = tmp_path / f"trials_{case}"
    trials.write_text("".join(f"s{a} t{b} {'target' if t else 'nontarget'}\n" for a, b, t in zip(ie, it, target)))
    return enroll, test, cohort, ie, it, target, u2e, u2t, spk2utt, str(trials)


def _device_vs_recorded_bounds(enroll, test, cohort, ie, it):
    C, D = cohort.shape
    k = min(200, C)
    me, se, ae = ref64_asv.cohort_topk_stats(enroll, cohort, k)
    mt, st, at = ref64_asv.cohort_topk_stats(test, cohort, k)
    s64, as64, aux = ref64_asv.trial_scores(enroll, test, ie, it, (me, se, mt, st))
    ds = ref64_asv.score_bound(s64, aux, D)
    dstats = (ref64_asv.topk_mean_bound(ae, C, D, k)[0], ref64_asv.topk_std_bound(ae, se, C, D, k),
              ref64_asv.topk_mean_bound(at, C, D, k)[0], ref64_asv.topk_std_bound(at, st, C, D, k))
    return s64, as64, ds, ref64_asv.asnorm_bound(s64, ds, (me, se, mt, st), dstats, ie, it)


@pytest.mark.parametrize("case", ("c50_t300", "c1000_t5000"))
def test_compute_metrics_against_the_references_recorded_scores(case, tmp_path):
    """scores and s-norm scores of the device against the reference's recorded ones: each side is a float32 evaluation within the
    derived bound of the float64 value, so they are within twice the bound of each other (and the device within once of float64)."""
    from satools_amd import asv_eval
    fx = np.load(os.path.join(GOLD, "fx_asv_eval.npz"))
    enroll, test, cohort, ie, it, target, u2e, u2t, spk2utt, trials = _fixture_case(fx, case, tmp_path)
    s64, as64, ds, das = _device_vs_recorded_bounds(enroll, test, cohort, ie, it)
    out = tmp_path / ("out_" + case)
    m = asv_eval.compute_metrics(u2e, u2t, spk2utt, trials, str(out), cohort=cohort)
    lines = [l.split() for l in open(out / "scores")]
    assert [(l[0], l[1]) for l in lines] == [(f"s{a}", f"t{b}") for a, b in zip(ie, it)]
    score = torch.tensor([float(l[2]) for l in lines], dtype=torch.float64)
    _check("compute_metrics scores", case + " vs float64", score, s64, ds)
    _check("compute_metrics scores", case + " vs recorded", score, torch.from_numpy(fx[case + "/scores"]), 2 * ds)
    dscore, dscore_as = asv_eval.score_trials(u2e, u2t, spk2utt, [l[0] for l in lines], [l[1] for l in lines], cohort=cohort)
    assert np.array_equal(dscore.astype(np.float64), score.numpy())          # the file holds the float32 scores exactly
    _check("compute_metrics asnorm", case + " vs float64", torch.from_numpy(dscore_as), as64, das)
    _check("compute_metrics asnorm", case + " vs recorded", torch.from_numpy(dscore_as), torch.from_numpy(fx[case + "/asnorm"]), 2 * das)
    assert set(m) == {"linkability", "eer", "eer_lower", "eer_upper", "min_cllr", "eer_threshold", "asnorm", "score"}
    assert set(m["asnorm"]) == {"linkability", "eer", "eer_lower", "eer_upper", "min_cllr", "eer_threshold"}
    assert len(m["score"][0]) == int(target.sum()) and len(m["score"][1]) == int((~target).sum())
    if case != "c50_t300":
        return
    # The metrics are functions of the ORDER of the scores (PAV, ROCCH) and of their histogram counts (linkability: with equal counts
    # the bin width cancels between density and trapezoid rule).  The fixture generator chose this case so that no target / non-target
    # pair and no score / bin-edge pair is closer than a margin; where that margin exceeds twice the distance the device may be from the
    # recorded scores, order and counts cannot differ and the metrics agree to float64 rounding: n 2^-52.
    try:
        import feerci  # noqa: F401
        have_feerci = True
    except ImportError:
        have_feerci = False
    for tag, rec, delta, got in (("raw", fx[case + "/scores"], 2 * float(ds.max()), m), ("as", fx[case + "/asnorm"].astype(np.float64), 2 * float(das.max()), m["asnorm"])):
        gap = np.abs(rec[target][:, None] - rec[~target][None, :]).min()
        edges = np.linspace(rec.min(), rec.max(), min(int(target.sum() / 10), 100) + 1)[1:-1]
        edge_gap = np.abs(rec[:, None] - edges[None, :]).min()
        print(f"{case} {tag}: smallest target / non-target gap {gap:.3e}, to a bin edge {edge_gap:.3e}, device may move a score by {delta:.3e}")
        assert gap > 2 * delta and edge_gap > 2 * delta, "the fixture no longer separates what the comparison needs separated"
        tol = len(rec) * 2.0 ** -52
        assert abs(got["linkability"] - float(fx[f"{case}/{tag}/linkability"])) <= tol
        assert abs(got["min_cllr"] - float(fx[f"{case}/{tag}/min_cllr"])) <= tol
        if not have_feerci:
            assert abs(got["eer"] - 100 * float(fx[f"{case}/{tag}/eer"])) <= 100 * tol
            assert got["eer_lower"] is None and got["eer_upper"] is None


# ---- test_metrics on a toy data directory ----------------------------------------------------------------------------------
def test_test_metrics_on_a_toy_directory(tmp_path):
    import satools_amd
    from satools_amd import asv_eval, pipeline, synthetic
    model = satools_amd.load_model("synthetic:xvector?speakers=12").to(DEV)
    wavs = tmp_path / "wav"
    wavs.mkdir()
    enroll = {"spkA-u1": 0, "spkA-u2": 1, "spkB-u1": 2, "spkC-u1": 3, "spkC-u2": 4, "spkC-u3": 5}
    trial = {"spkA-u2": 1, "spkA-t1": 6, "spkB-t1": 7, "spkC-t1": 8, "spkB-t2": 9}         # spkA-u2 is in both lists
    for name, seed in {**enroll, **trial}.items():
        pipeline.save_pcm16(wavs / (name + ".wav"), synthetic.harm_utterance(seed, 16000 + 1601 * seed).unsqueeze(0), 16000)
    (tmp_path / "enroll.scp").write_text("".join(f"{n} {wavs / (n + '.wav')}\n" for n in enroll))
    (tmp_path / "trials.scp").write_text("".join(f"{n} {wavs / (n + '.wav')}\n" for n in trial))
    (tmp_path / "utt2spk").write_text("".join(f"{n} {n.split('-')[0]}\n" for n in enroll))
    tl = [(s, u, "target" if u.startswith(s) else "nontarget") for s in ("spkA", "spkB", "spkC") for u in trial]
    (tmp_path / "trials").write_text("".join(" ".join(t) + "\n" for t in tl))
    calls = []
    fwd = model.forward
    model.forward = lambda x, target=None: (calls.append(int(x.shape[-1])), fwd(x, target=target))[1]
    out = tmp_path / "out"
    m = asv_eval.test_metrics(model, str(tmp_path / "enroll.scp"), str(tmp_path / "trials.scp"), str(tmp_path / "utt2spk"),
                              str(tmp_path / "trials"), str(out))
    assert len(calls) == len(set(enroll) | set(trial)) == 10                  # the shared utterance is extracted once
    z = np.load(out / "xvectors.npz")
    xv = {str(u): torch.from_numpy(v) for u, v in zip(z["utts"], z["xvectors"])}
    assert set(xv) == set(enroll) | set(trial) and z["xvectors"].shape == (10, 192)
    spk2utt = {}
    for n in enroll:
        spk2utt.setdefault(n.split("-")[0], []).append(n)
    speakers = list(spk2utt)
    rows = [u for s in speakers for u in spk2utt[s]]
    offsets = np.concatenate([[0], np.cumsum([len(spk2utt[s]) for s in speakers])])
    X = torch.stack([xv[u] for u in rows])
    e64, eaux = ref64_asv.segment_mean_l2norm(X, np.arange(len(rows)), offsets)
    de = ref64_asv.segment_bound(e64, eaux, 192).norm(dim=1)                   # the enrolment vector's own error, as a 2-norm
    tn = list(trial)
    T = torch.stack([xv[u] for u in tn])
    ie = [speakers.index(s) for s, _, _ in tl]
    it = [tn.index(u) for _, u, _ in tl]
    s64, _, aux = ref64_asv.trial_scores(e64, T, ie, it)
    # a perturbation da of a unit vector a moves its cosine with anything by at most 2 |da|
    bound = ref64_asv.score_bound(s64, aux, 192) + 2 * de[torch.as_tensor(ie)]
    lines = [l.split() for l in open(out / "scores")]
    assert [(l[0], l[1]) for l in lines] == [(s, u) for s, u, _ in tl]
    _check("test_metrics scores", "toy directory", torch.tensor([float(l[2]) for l in lines], dtype=torch.float64), s64, bound)
    mj = json.load(open(out / "metric.json"))
    keys = {"linkability", "eer", "eer_lower", "eer_upper", "min_cllr", "eer_threshold"}
    assert set(mj) == keys | {"asnorm"} and set(mj["asnorm"]) == keys
    assert mj["asnorm"]["eer"] is not None and m["eer"] == mj["eer"]           # the cohort of 12 speakers was used (k = 12)
