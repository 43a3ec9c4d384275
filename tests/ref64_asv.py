"""Float64 restatements of the ASV scoring kernels (csrc/asv_score.hip), written from the formulas of the reference's
sidekit/scoring/__init__.py (asnorm, cosine_scoring) and sidekit/objf.py:272-281 (per-speaker enrolment vectors), in float64 torch
on the CPU.  Each function also returns the sums of absolute terms its rounding-error bound needs.  A plain module: no fixtures,
no GPU.  tests/test_asv_host.py pins it against the reference's recorded outputs (tests/golden/fx_asv_eval.npz).

ERROR MODEL (U = 2^-24, k(n) = ref64.reduction_terms(n) = ceil(n / 64) + 8 roundings for a wave-wide sum of n terms):
  * one score x . c:            E = k(D) U sum_d |x_d c_d|
  * the k largest of C scores:  two score sets that differ by at most E elementwise have sorted top-k lists that differ by at most
                                E elementwise (the j-th largest is a 1-Lipschitz function of the set in the max norm), whatever the
                                ties at the k-th place.  So |d mean| <= E and, the deviation being the 2-norm of the centred list
                                over sqrt(k - 1), |d std| <= E sqrt(k / (k - 1)).
  * the k-term sums on top:     `stat_roundings(C, k)` roundings of size U sum |v| for the mean (a lane adds at most
                                min(k, 4 ceil(C / 256)) selected values one by one, six shuffle levels, then the multiply by the
                                repeat count, the add of that product and the division); for the deviation `topk_std_bound`, which
                                adds to E sqrt(k / (k - 1)) only roundings of its own arithmetic."""
import contextlib
import math

import torch

from ref64 import U, reduction_terms

_DT = torch.float64


def _d(x):
    return torch.as_tensor(x).detach().cpu().to(_DT)


@contextlib.contextmanager
def in_float32():
    """evaluate the same formulas in float32 torch on the CPU (the reference's own precision)"""
    global _DT
    _DT = torch.float32
    try:
        yield
    finally:
        _DT = torch.float64


def stat_roundings(C, k):
    return min(k, 4 * math.ceil(C / 256)) + 6 + 3


# ---- asnorm's statistics, per vector -----------------------------------------------------------------------------------
def cohort_topk_stats(x, cohort, k):
    """x [N, D], cohort [C, D] -> (mean [N], std [N]) of the k largest of the C dot products of each row; std unbiased (NaN for
    k = 1).  aux: "S" [N] = max over the cohort of sum_d |x_d c_d| (the score error of the row is k(D) U S), "A" [N] = sum of the
    |values| of the top k, "topk" [N, k]"""
    x, cohort = _d(x), _d(cohort)
    scores = x @ cohort.t()
    top = scores.topk(k, dim=1).values
    mean = top.mean(dim=1)
    std = top.std(dim=1) if k > 1 else torch.full_like(mean, float("nan"))
    S = (x.abs() @ cohort.abs().t()).max(dim=1).values
    return mean, std, {"S": S, "A": top.abs().sum(dim=1), "topk": top}


def topk_mean_bound(aux, C, D, k):
    """|device mean - float64 mean| <= E + roundings of the k-term sum"""
    E = reduction_terms(D) * U * aux["S"].double()
    return E + stat_roundings(C, k) * U * aux["A"].double() / k, E


def topk_std_bound(aux, std, C, D, k):
    """|device std - float64 std|: the scores (E sqrt(k / (k - 1)): the deviation of the device's own top-k list around that list's own
    mean), the ROUNDING error dm of the device's mean around its own scores (sum (v - m')^2 = sum (v - m)^2 + k (m - m')^2, so at most
    sqrt(k / (k - 1)) dm on the std; dm = stat_roundings U A / k, the score error E is not in it), and the arithmetic: every deviation
    rounded (2 U on its square), the square (U), the sum (stat_roundings), the product with the repeat count (2 U), the division and
    the square root (U each, halved through the root for the first)"""
    E = reduction_terms(D) * U * aux["S"].double()
    dm = stat_roundings(C, k) * U * aux["A"].double() / k
    r = math.sqrt(k / (k - 1.0))
    rel = (stat_roundings(C, k) + 3 + 2 + 1) / 2.0 * U + U
    return E * r + dm * r + rel * std.double()


# ---- cosine score and s-norm of a trial ------------------------------------------------------------------------------
def trial_scores(enroll, test, idx_e, idx_t, stats=None):
    """score[m] = a . b / (|a| |b|), a = enroll[idx_e[m]], b = test[idx_t[m]]; with stats = (mu_e, sd_e, mu_t, sd_t) also
    ((s - mu_e) / sd_e + (s - mu_t) / sd_t) / 2 with the statistics gathered per trial.
    aux: "Sab" = sum |a_d b_d|, "Saa", "Sbb" (= |a|^2, |b|^2) per trial"""
    a = _d(enroll)[torch.as_tensor(idx_e).long()]
    b = _d(test)[torch.as_tensor(idx_t).long()]
    ab, aa, bb = (a * b).sum(1), (a * a).sum(1), (b * b).sum(1)
    s = ab / (aa.sqrt() * bb.sqrt())
    aux = {"Sab": (a * b).abs().sum(1), "Saa": aa, "Sbb": bb}
    if stats is None:
        return s, None, aux
    mu_e, sd_e, mu_t, sd_t = (_d(t) for t in stats)
    ie, it = torch.as_tensor(idx_e).long(), torch.as_tensor(idx_t).long()
    return s, 0.5 * ((s - mu_e[ie]) / sd_e[ie] + (s - mu_t[it]) / sd_t[it]), aux


def score_bound(score, aux, D):
    """|device score - float64 score|: the three sums (k(D) U S each), two square roots, their product and the division"""
    k = reduction_terms(D)
    s = score.double().abs()
    dab = k * U * aux["Sab"].double()
    nrm = (aux["Saa"].double() * aux["Sbb"].double()).sqrt().clamp(min=1e-300)
    return dab / nrm + s * (k * U + 4 * U)          # d|a|/|a| = k U / 2 for each norm, + sqrt, sqrt, multiply, divide


def asnorm_bound(score, ds, stats, dstats, idx_e, idx_t):
    """first order per element: sum over the two sides of ((ds + dmu) / sd + |s - mu| dsd / sd^2) / 2, + the roundings of the formula
    itself (subtract, divide per side, add, halve: 3 U of each term and U of the result)"""
    ie, it = torch.as_tensor(idx_e).long(), torch.as_tensor(idx_t).long()
    s = score.double()
    out = torch.zeros_like(s)
    mag = torch.zeros_like(s)
    for (mu, sd), (dmu, dsd), ix in ((stats[0:2], dstats[0:2], ie), (stats[2:4], dstats[2:4], it)):
        mu, sd, dmu, dsd = mu.double()[ix], sd.double()[ix], dmu.double()[ix], dsd.double()[ix]
        out = out + 0.5 * ((ds + dmu) / sd + (s - mu).abs() * dsd / sd ** 2)
        mag = mag + 0.5 * (s - mu).abs() / sd
    return out + 4 * U * mag


# ---- per-speaker enrolment vectors ------------------------------------------------------------------------------------
def segment_mean_l2norm(x, order, offsets):
    """x [U, D] -> [S, D]: the mean of the rows x[order[offsets[s]:offsets[s+1]]] over its L2 norm; a segment of one row is that row.
    aux: "S1" [S, D] = sum |x| of the segment per dimension, "n" [S], "mean" [S, D] (before the division), "nrm" [S]"""
    x = _d(x)
    order = [int(v) for v in order]
    offsets = [int(v) for v in offsets]
    out, S1, ns, means, nrms = [], [], [], [], []
    for s in range(len(offsets) - 1):
        rows = x[order[offsets[s]:offsets[s + 1]]]
        n = rows.shape[0]
        m = rows.sum(0) / n
        nrm = m.norm() if n > 1 else torch.ones((), dtype=_DT)
        out.append(m / nrm if n > 1 else rows[0])
        S1.append(rows.abs().sum(0)), ns.append(n), means.append(m), nrms.append(nrm)
    return torch.stack(out), {"S1": torch.stack(S1), "n": torch.tensor(ns), "mean": torch.stack(means), "nrm": torch.stack(nrms)}


def segment_bound(out, aux, D):
    """rows of several utterances: the mean of n rows (n roundings of U S1 / n, the division inside), its norm (k(D) U on the sum
    of squares -> half on the root, + the mean's own error through the norm: at most |dmean|_2), the final division.  Rows of one
    utterance: 0 (a copy)"""
    n = aux["n"].double().view(-1, 1)
    dmean = (n + 1) * U * aux["S1"].double() / n
    nrm = aux["nrm"].double().view(-1, 1).clamp(min=1e-300)
    dnrm = dmean.norm(dim=1, keepdim=True) + (reduction_terms(D) / 2.0 + 1) * U * nrm
    b = dmean / nrm + out.double().abs() * (dnrm / nrm + U)
    return torch.where(n > 1, b, torch.zeros_like(b))
