"""ASV privacy evaluation: how well does the anonymisation hide the speaker?
(reference: egs/anon/vctk/local/eval.py:196-231 -> satools/sidekit/model.py:208-239 `--mode eval` ->
satools/sidekit/objf.py:186-369 `test` / `compute_metrics` -> satools/sidekit/scoring/__init__.py:7-55 and scoring/metric.py)

`test_metrics` extracts the enrolment and trial x-vectors with an x-vector extractor of this package (ECAPA-TDNN or the half-ResNet34), `compute_metrics`
averages the enrolment vectors per speaker, cosine-scores the trial list, applies adaptive s-norm against a cohort and computes
linkability, min Cllr and the EER.  The arithmetic over vectors runs on the device (csrc/asv_score.hip):

  per-speaker enrolment vectors            ops.segment_mean_l2norm
  cohort statistics of adaptive s-norm     ops.cohort_topk_stats — once per unique speaker and per unique test utterance, not once
                                           per trial as the reference computes them; the score matrices never exist
  cosine score and s-norm of every trial   ops.trial_scores

The metrics are functions of the M scores alone and run on the host in float64 numpy: `linkability` (Gomez-Barrero et al. 2017, as
adapted by the reference's metric.py:10-68), `min_cllr` with the PAV calibration (Bruemmer & du Preez 2006; metric.py:250-535) and
the ROCCH-EER of that calibration.  They are written from the papers' formulae and the reference's conventions (bin rule, tie
order, the monotonicity ramp), with a linear-time stack PAV in place of the reference's Python loop.

EER: the reference takes `eer`, its bootstrap interval and the threshold from the third-party `feerci` package.  When `feerci` can be
imported it is called exactly as objf.py:332 calls it; otherwise `eer` is the ROCCH-EER x 100, `eer_threshold` the calibrated LLR of
the ROCCH segment that crosses the diagonal, and `eer_lower` / `eer_upper` are None (parity unpinned: INTEGRATION.md).  With
`eer_ci` (`asv-eval --eer-ci M`) the three come from `eer_interval` instead: the empirical EER of the calibrated LLRs and the percentile
interval of M bootstrap replicates of it, drawn and counted on the device (ops.eer_bootstrap, csrc/stats/eer_bootstrap.hip)."""
import json
import logging
import os

import numpy as np
import torch

from . import _lib, ops

TOP_K = 200          # scoring/__init__.py:26


# ---- metrics on the host (float64) ---------------------------------------------------------------------------------
def linkability(mated, non_mated, omega=1.0, n_bins=-1):
    """global linkability D_sys of two score sets -> (D_sys, D per bin, bin centres, bin edges).
    Bins: min(len(mated) // 10, 100) equal bins from the smallest to the largest score of both sets; local measure
    D = 2 w LR / (1 + w LR) - 1 where w LR > 1, else 0, with LR the ratio of the two normalised histograms (LR = 1 where the
    non-mated histogram is empty and the mated one too, D = 1 where only the non-mated one is); D_sys = trapezoid rule of D x the
    mated density over the bin centres."""
    mated = np.asarray(mated, dtype=np.float64)
    non_mated = np.asarray(non_mated, dtype=np.float64)
    if n_bins < 0:
        n_bins = min(int(len(mated) / 10), 100)
    if n_bins < 1:             # fewer than 10 mated scores: no bin, nothing to integrate (the reference's histogram call fails here)
        return 0.0, np.zeros(0), np.zeros(0), np.zeros(0)
    lo = min(mated.min(), non_mated.min())
    hi = max(mated.max(), non_mated.max())
    edges = np.linspace(lo, hi, num=n_bins + 1, endpoint=True)
    centres = (edges[1:] + edges[:-1]) / 2
    dens_m = np.histogram(mated, bins=edges, density=True)[0]
    dens_n = np.histogram(non_mated, bins=edges, density=True)[0]
    lr = np.ones_like(dens_m)
    has_n = dens_n != 0
    lr[has_n] = dens_m[has_n] / dens_n[has_n]
    wlr = omega * lr
    local = 2 * (wlr / (1 + wlr)) - 1
    local[wlr <= 1] = 0
    local[(~has_n) & (dens_m != 0)] = 1
    f = local * dens_m
    d_sys = float(np.sum((centres[1:] - centres[:-1]) * (f[1:] + f[:-1]) / 2.0)) if len(centres) > 1 else 0.0
    return d_sys, local, centres, edges


def pav(y):
    """pool adjacent violators: the non-decreasing fit of y that is closest in squares -> (fit [n], block widths, block heights).
    One pass with a stack of (sum, count) blocks: a new point is a block; while the block below is not lower it is merged in."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    if y.ndim != 1 or n == 0:
        raise ValueError("pav: a non-empty vector is needed")
    sums = np.empty(n)
    counts = np.empty(n, dtype=np.int64)
    top = -1
    for v in y.tolist():
        top += 1
        sums[top], counts[top] = v, 1
        # (means compared as s_a n_b >= s_b n_a: exact for the 0 / 1 labels of the calibration)
        while top > 0 and sums[top - 1] * counts[top] >= sums[top] * counts[top - 1]:
            sums[top - 1] += sums[top]
            counts[top - 1] += counts[top]
            top -= 1
    widths = counts[:top + 1].copy()
    heights = sums[:top + 1] / widths
    return np.repeat(heights, widths), widths, heights


def _logit(p):
    out = np.empty_like(p)
    mid = (p > 0) & (p < 1)
    out[mid] = np.log(p[mid] / (1 - p[mid]))
    out[p <= 0] = -np.inf
    out[p >= 1] = np.inf
    return out


def cllr(tar_llrs, non_llrs):
    """application-independent cost of log-likelihood ratios, in bits (Bruemmer & du Preez 2006)"""
    with np.errstate(over="ignore", divide="ignore"):
        p_tar = 1 / (1 + np.exp(-np.asarray(tar_llrs, dtype=np.float64)))
        p_non = 1 / (1 + np.exp(np.asarray(non_llrs, dtype=np.float64)))
        if np.any(p_tar == 0) or np.any(p_non == 0):
            return float("inf")
        ln2 = np.log(2)
        return float(((-np.log(p_tar)).mean() / ln2 + (-np.log(p_non)).mean() / ln2) / 2)


def calibrate(tar, non, monotonicity_epsilon=1e-6):
    """optimal (PAV) calibration of two score sets -> dict: tar_llrs / non_llrs (in the input order), eer = the ROCCH-EER as a
    fraction, eer_threshold = the calibrated LLR of the ROCCH segment that crosses the diagonal.
    Scores are sorted stably with the non-targets first among ties; the ideal posteriors (0 / 1 labels) are fitted by `pav`,
    turned into log-odds, the prior log-odds len(tar) / len(non) taken off, and a ramp of epsilon i / N added to keep them
    strictly ordered.  The ROC convex hull has one vertex per PAV block boundary; its EER is the largest diagonal crossing
    det / (dy + dx) over the hull's segments, axis-parallel segments counting as 0."""
    tar = np.asarray(tar, dtype=np.float64)
    non = np.asarray(non, dtype=np.float64)
    n_tar, n_non = len(tar), len(non)
    n = n_tar + n_non
    scores = np.concatenate([non, tar])
    labels = np.concatenate([np.zeros(n_non), np.ones(n_tar)])
    order = np.argsort(scores, kind="mergesort")
    labels = labels[order]
    fit, widths, heights = pav(labels)
    with np.errstate(divide="ignore"):
        prior = np.log(n_tar / n_non)
        llrs = _logit(fit) - prior
        block_llrs = _logit(heights) - prior
    llrs = llrs + np.arange(n) * monotonicity_epsilon / n
    back = np.empty(n, dtype=np.int64)
    back[order] = np.arange(n)
    llrs = llrs[back]
    # ROCCH vertices: threshold to the left of block i -> i scores-blocks rejected
    left = np.concatenate([[0], np.cumsum(widths)])
    tar_below = np.concatenate([[0.0], np.cumsum(labels)])[left]              # targets rejected: misses
    non_above = (n - left) - (n_tar - tar_below)                              # non-targets accepted: false alarms
    pmiss = tar_below / n_tar
    pfa = non_above / n_non
    x0, x1, y0, y1 = pfa[:-1], pfa[1:], pmiss[:-1], pmiss[1:]
    if not (np.all(x1 <= x0) and np.all(y0 <= y1)):
        raise AssertionError("ROCCH vertices are not ordered")
    dx, dy = x0 - x1, y1 - y0
    live = (dx != 0) & (dy != 0)
    cross = np.zeros(len(dx))
    cross[live] = (x0[live] * y1[live] - x1[live] * y0[live]) / (dy[live] + dx[live])
    eer = float(cross.max()) if len(cross) else 0.0
    thr = float(block_llrs[int(np.argmax(cross))]) if eer > 0 else 0.0
    return {"tar_llrs": llrs[n_non:], "non_llrs": llrs[:n_non], "eer": max(eer, 0.0), "eer_threshold": thr}


def min_cllr(tar, non, monotonicity_epsilon=1e-6):
    """Cllr of the optimally calibrated scores -> (min Cllr, ROCCH-EER, calibrated target LLRs, calibrated non-target LLRs)"""
    c = calibrate(tar, non, monotonicity_epsilon)
    return cllr(c["tar_llrs"], c["non_llrs"]), c["eer"], c["tar_llrs"], c["non_llrs"]


# ---- the empirical EER and its bootstrap interval ------------------------------------------------------------------
def eer_cuts(tar_sorted, non_sorted):
    """the two sorted score sets as integer cut tables over the K distinct values v_0 < ... < v_{K-1} of both together, +inf as index K:
    cut_tar[k] = #{tar < v_k}, cut_non[k] = #{non < v_k}, cut_*[K] = n_* -> (cut_tar [K + 1], cut_non [K + 1]) int32.
    The EER depends on the sets through these tables alone."""
    tar = np.asarray(tar_sorted, dtype=np.float64)
    non = np.asarray(non_sorted, dtype=np.float64)
    if tar.ndim != 1 or non.ndim != 1 or tar.size == 0 or non.size == 0:
        raise ValueError("eer_cuts: two non-empty score vectors are needed")
    if np.isnan(tar).any() or np.isnan(non).any():
        raise ValueError("eer_cuts: NaN scores have no order")
    if np.any(np.diff(tar) < 0) or np.any(np.diff(non) < 0):
        raise ValueError("eer_cuts: the score vectors must be sorted")
    v = np.unique(np.concatenate([tar, non]))
    cut_tar = np.append(np.searchsorted(tar, v, side="left"), tar.size).astype(np.int32)
    cut_non = np.append(np.searchsorted(non, v, side="left"), non.size).astype(np.int32)
    return cut_tar, cut_non


def _eer_from_cuts(cut_tar, cut_non):
    n_tar, n_non = int(cut_tar[-1]), int(cut_non[-1])
    miss = cut_tar.astype(np.int64)
    fa = n_non - cut_non.astype(np.int64)
    k = int(np.argmax(miss * n_non >= fa * n_tar))            # the first threshold at which the misses have caught up: 1 <= k <= K
    m, f = int(miss[k]), int(fa[k - 1])
    return min(m / n_tar, f / n_non), m, f


def empirical_eer(tar, non):
    """the equal error rate of the two score sets as they are, no convex hull -> (eer, miss_count, fa_count).
    A trial is accepted when score >= t; t runs over the K distinct values of both sets and +inf (index K).  miss(k) = #{tar < v_k} never
    decreases, fa(k) = #{non >= v_k} never increases, miss(0) = 0 and fa(K) = 0.  With k* the smallest k at which miss(k) n_non >=
    fa(k) n_tar (int64 products: no rounding decides it),  EER = min(miss(k*) / n_tar, fa(k* - 1) / n_non) = min_t max(P_miss(t), P_fa(t)).
    Thresholds sit on distinct values, so ties are safe.  Never smaller than the ROCCH-EER of `calibrate`."""
    ct, cn = eer_cuts(np.sort(np.asarray(tar, dtype=np.float64)), np.sort(np.asarray(non, dtype=np.float64)))
    return _eer_from_cuts(ct, cn)


def eer_interval(tar, non, m=10000, ci=0.95, seed=0, device=None):
    """the empirical EER and the percentile interval of m bootstrap replicates of it -> (eer, lower, upper, replicate_eers [m]), fractions.
    Replicate r resamples both sets with replacement (ops.eer_bootstrap: Philox4x32-10 draws, a function of (seed, r) alone; the index
    mapping (u n) >> 32 is biased by at most n / 2^32 relative between two indices, 2.4e-4 at n = 2^20) and the device returns its two
    integer counts; the two divisions and the min are float64 here.  lower / upper = np.percentile(replicates, [50 (1 - ci), 50 (1 + ci)])
    with numpy's default linear rule.  feerci's own percentile and tie rules are not known here: parity with feerci stays unpinned."""
    if not 0 < ci < 1:
        raise ValueError(f"eer_interval: ci = {ci} outside (0, 1)")
    tar = np.sort(np.asarray(tar, dtype=np.float64))
    non = np.sort(np.asarray(non, dtype=np.float64))
    ct, cn = eer_cuts(tar, non)
    eer = _eer_from_cuts(ct, cn)[0]
    miss, fa = ops.eer_bootstrap(ct, cn, tar.size, non.size, m, seed=seed, device=device)
    reps = np.minimum(miss.cpu().numpy().astype(np.float64) / tar.size, fa.cpu().numpy().astype(np.float64) / non.size)
    # 50 (1 -+ ci) as 50 -+ 50 ci: 1 - 0.95 is not 0.05 in float64 (50 (1 - 0.95) = 2.500000000000002, and the interpolated percentile moves
    # by an ulp), while 50 - 50 * 0.95 is 2.5
    lower, upper = np.percentile(reps, [50 - 50 * ci, 50 + 50 * ci])
    return eer, float(lower), float(upper), reps


def score_metrics(mated, non_mated, eer_ci=None):
    """the reference's metric set of one pair of score sets (objf.py:330-339) -> (dict, calibrated mated, calibrated non-mated).
    eer_ci = dict(m=replicates, ci=0.95, seed=0[, device]): without feerci, `eer`, `eer_lower` and `eer_upper` (x 100) come from
    `eer_interval` of the calibrated LLRs, the arguments the reference hands to feerci.  The reference takes all three from one routine, so
    `eer` is then the EMPIRICAL EER, not the ROCCH-EER (which is never larger).  `eer_threshold` and the key set do not change, and
    feerci, when it can be imported, still wins."""
    d_sys = linkability(mated, non_mated)[0]
    c = calibrate(mated, non_mated)
    cmin = cllr(c["tar_llrs"], c["non_llrs"])
    try:
        from feerci import feerci
    except ImportError:
        eer, lower, upper, thr = c["eer"] * 100, None, None, c["eer_threshold"]
        if eer_ci is not None:
            e, lo, up, _ = eer_interval(c["tar_llrs"], c["non_llrs"], **eer_ci)
            eer, lower, upper = e * 100, lo * 100, up * 100
    else:
        eer, lower, upper, _boot, thr = feerci(c["non_llrs"], c["tar_llrs"], is_sorted=False, return_threshold=True)
        eer, lower, upper, thr = float(eer * 100), float(lower * 100), float(upper * 100), float(thr)
    return ({"linkability": d_sys, "eer": eer, "eer_lower": lower, "eer_upper": upper, "min_cllr": cmin, "eer_threshold": thr},
            c["tar_llrs"], c["non_llrs"])


# ---- scoring on the device -----------------------------------------------------------------------------------------
def read_trials(trials_file):
    """`enrol-speaker test-utterance target|nontarget` per line -> (speakers, utterances, labels)"""
    spk, utt, lab = [], [], []
    with open(trials_file) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if len(t) < 3:
                raise _lib.SatError(f"{trials_file}: a trial line needs `enrol test target|nontarget`, got '{line.strip()}'")
            spk.append(t[0]), utt.append(t[1]), lab.append(t[2])
    if not spk:
        raise _lib.SatError(f"{trials_file}: no trials")
    return spk, utt, lab


def _stack(vectors, device):
    """vectors of one length, all on one device -> [n, D] float32 on `device` (one stack, one copy)"""
    rows = [torch.as_tensor(v).detach().reshape(-1) for v in vectors]
    if len({r.device for r in rows}) > 1:
        rows = [r.to(device) for r in rows]
    return torch.stack(rows).to(device=device, dtype=torch.float32).contiguous()


def score_trials(utt2embd_enroll, utt2embd_trial, enroll_spk2utt, spk_of_trial, utt_of_trial, cohort=None, device=None):
    """-> (score [M], score_asnorm [M] or None) as float32 numpy arrays, in trial order.  Every enrolment speaker and every
    distinct test utterance is one row on the device; the trial list only carries their row numbers."""
    if device is None:
        first = next(iter(utt2embd_enroll.values()))
        device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device("cuda")
    speakers = list(enroll_spk2utt)
    order_utts, offsets = [], [0]
    for s in speakers:
        utts = enroll_spk2utt[s]
        if not utts:
            raise _lib.SatError(f"enrolment speaker {s} has no utterance")
        order_utts += utts
        offsets.append(len(order_utts))
    missing = [u for u in order_utts if u not in utt2embd_enroll]
    if missing:
        raise _lib.SatError(f"no enrolment x-vector for {missing[:3]}{' ...' if len(missing) > 3 else ''}")
    enroll = ops.segment_mean_l2norm(_stack([utt2embd_enroll[u] for u in order_utts], device), np.arange(len(order_utts)), offsets)
    spk_row = {s: i for i, s in enumerate(speakers)}
    utt_row = {}
    for u in utt_of_trial:
        if u not in utt_row:
            if u not in utt2embd_trial:
                raise _lib.SatError(f"no trial x-vector for {u}")
            utt_row[u] = len(utt_row)
    unknown = [s for s in spk_of_trial if s not in spk_row]
    if unknown:
        raise _lib.SatError(f"the trial list names speakers without enrolment: {unknown[:3]}")
    test = _stack([utt2embd_trial[u] for u in utt_row], device)
    idx_e = np.fromiter((spk_row[s] for s in spk_of_trial), dtype=np.int32, count=len(spk_of_trial))
    idx_t = np.fromiter((utt_row[u] for u in utt_of_trial), dtype=np.int32, count=len(utt_of_trial))
    if cohort is None:
        return ops.trial_scores(enroll, test, idx_e, idx_t).cpu().numpy(), None
    cohort = torch.as_tensor(cohort).detach().to(device=device, dtype=torch.float32).contiguous()
    k = min(TOP_K, cohort.shape[0])
    mu_e, sd_e = ops.cohort_topk_stats(enroll, cohort, k)
    mu_t, sd_t = ops.cohort_topk_stats(test, cohort, k)
    score, score_as = ops.trial_scores(enroll, test, idx_e, idx_t, (mu_e, sd_e, mu_t, sd_t))
    return score.cpu().numpy(), score_as.cpu().numpy()


def compute_metrics(utt2embd_enroll, utt2embd_trial, enroll_spk2utt, trials_file, out_scores, cohort=None, device=None, eer_ci=None):
    """objf.py:268-369: x-vectors by utterance, the enrolment speakers' utterance lists, the trial list -> the metric dict
    (`linkability`, `eer`, `eer_lower`, `eer_upper`, `min_cllr`, `eer_threshold`, `asnorm` = the same six after adaptive s-norm
    against `cohort` (None without one), `score` = the calibrated (mated, non-mated) LLRs of the last set computed).
    Writes `<out_scores>/scores`: `enrol test score` per trial.  eer_ci: see `score_metrics`."""
    spk, utt, lab = read_trials(trials_file)
    if eer_ci is not None and "device" not in eer_ci:
        eer_ci = dict(eer_ci, device=device)
    score, score_as = score_trials(utt2embd_enroll, utt2embd_trial, enroll_spk2utt, spk, utt, cohort=cohort, device=device)
    os.makedirs(out_scores, exist_ok=True)
    with open(os.path.join(out_scores, "scores"), "w") as f:
        for s, u, v in zip(spk, utt, score.tolist()):
            f.write(f"{s} {u} {v!r}\n")
    lab = np.asarray(lab)
    tar, non = lab == "target", lab == "nontarget"
    if not tar.any() or not non.any():
        raise _lib.SatError(f"{trials_file}: the metrics need target and nontarget trials")
    metrics, mated, non_mated = score_metrics(score[tar].astype(np.float64), score[non].astype(np.float64), eer_ci=eer_ci)
    metrics["asnorm"] = {k: None for k in ("eer", "linkability", "eer_lower", "eer_upper", "min_cllr", "eer_threshold")}
    if score_as is not None:
        m_as, mated, non_mated = score_metrics(score_as[tar].astype(np.float64), score_as[non].astype(np.float64), eer_ci=eer_ci)
        metrics["asnorm"].update(m_as)
    metrics["score"] = (mated, non_mated)
    return metrics


_logged_no_batch = set()


def extract_xvectors(model, enroll_scp, trials_scp, device, batch_size=1, max_frames=65536):
    """the extraction step of `test_metrics`: two {utterance: scp entry} dicts -> two {utterance: x-vector [D]} dicts in their order; an
    utterance of both lists is extracted once.  batch_size = 1, or a model without `extract_batch`: `model(wav)` per utterance; otherwise
    ragged groups through `model.extract_batch` (both extractors of this package have it)."""
    from .pipeline import load_wav_from_scp

    def extract(entry):
        wav, _sr = load_wav_from_scp(entry)
        with torch.no_grad():
            _, xv = model(wav.squeeze().to(device), target=None)
        return xv.reshape(-1)

    batched = int(batch_size) > 1 and hasattr(model, "extract_batch")
    if int(batch_size) > 1 and not batched and type(model).__qualname__ not in _logged_no_batch:
        _logged_no_batch.add(type(model).__qualname__)
        logging.getLogger(__name__).warning("batch_size = %d: this extractor has no extract_batch, one utterance per call", int(batch_size))
    if not batched:
        enroll = {u: extract(e) for u, e in enroll_scp.items()}
        return enroll, {u: enroll[u] if u in enroll else extract(e) for u, e in trials_scp.items()}
    # scp order, up to batch_size utterances and up to max_frames frames per call (a longer utterance is a call of its own); the samples
    # of one group at a time are in host memory
    todo = list(enroll_scp.items()) + [(u, e) for u, e in trials_scp.items() if u not in enroll_scp]
    vec, group, total = {}, [], 0

    def flush():
        with torch.no_grad():
            xv = model.extract_batch([w.to(device) for _, w in group])
        for row, (u, _) in enumerate(group):
            vec[u] = xv[row].reshape(-1)

    for u, e in todo:
        wav = load_wav_from_scp(e)[0].reshape(-1)
        frames = 1 + int(wav.shape[0]) // 160
        if group and (len(group) >= int(batch_size) or total + frames > int(max_frames)):
            flush()
            group, total = [], 0
        group.append((u, wav))
        total += frames
    if group:
        flush()
    return {u: vec[u] for u in enroll_scp}, {u: vec[u] for u in trials_scp}


def test_metrics(model, enroll_wav_scp, trials_wav_scp, enroll_utt2spk, trials_file, out_dir, as_norm=True, eer_ci=None, batch_size=1,
                 max_frames=65536):
    """objf.py:189-266: extract, score, measure.  Writes `<out_dir>/xvectors.npz` (`utts`, `xvectors`), `scores` and `metric.json`
    and returns the metric dict.  batch_size = 1: one utterance per extractor call, as the reference (the row kernels take no
    per-utterance lengths, and zero padding would change the InstanceNorm and the pooling).  batch_size = N > 1 with a model that has
    `extract_batch` (the ECAPA-TDNN net and the ResNet net): the utterances, in scp order, go N at a time — and at most `max_frames`
    frames at a time — through one ragged call each (xvector.Net.extract_batch, xvector_resnet.Net.extract_batch).  Memory of a call:
    the ECAPA net's 1 536-channel buffer of 65 536 frames is 403 MB; the ResNet's first images, [32][80][frames], are 10 KB per frame —
    671 MB at 65 536 frames, several of them live at once: lower `max_frames` where that does not fit.  A model without `extract_batch`
    extracts one per call and says so once.  An utterance of both lists is extracted once either way.
    eer_ci: see `score_metrics`."""
    from .pipeline import read_wav_scp
    model.eval()
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise _lib.SatError("x-vector extraction runs on the HIP device only: move the model there first (no CPU fallback)")
    if int(batch_size) < 1 or int(max_frames) < 1:
        raise _lib.SatError(f"test_metrics: batch_size = {batch_size}, max_frames = {max_frames}: both at least 1")
    enroll_scp, trials_scp = read_wav_scp(enroll_wav_scp), read_wav_scp(trials_wav_scp)
    spk2utt = {}
    for u, s in read_wav_scp(enroll_utt2spk).items():
        spk2utt.setdefault(s, []).append(u)

    enroll, trial = extract_xvectors(model, enroll_scp, trials_scp, device, batch_size=batch_size, max_frames=max_frames)
    cohort = None
    if as_norm and hasattr(model, "after_speaker_embedding"):
        cohort = torch.nn.functional.normalize(model.after_speaker_embedding.weight.data, dim=1)
    os.makedirs(out_dir, exist_ok=True)
    both = dict(enroll)
    both.update(trial)
    np.savez(os.path.join(out_dir, "xvectors.npz"), utts=np.asarray(list(both)),
             xvectors=torch.stack(list(both.values())).cpu().numpy())
    metrics = compute_metrics(enroll, trial, spk2utt, trials_file, out_dir, cohort=cohort, device=device, eer_ci=eer_ci)
    with open(os.path.join(out_dir, "metric.json"), "w") as f:
        json.dump({k: v for k, v in metrics.items() if k != "score"}, f, indent=1)
    return metrics


test_metrics.__test__ = False      # (a library function, not a pytest case)


def report_lines(metrics):
    """the two lines of the reference's report step (eval.py:87-96 print_asv_metrics) from a metric dict: raw scores, then adaptive s-norm
    (left out when there was no cohort).  The half-width (upper - lower) / 2 of the interval, to 3 places, follows the EER when there is
    an interval and is omitted when `eer_lower` / `eer_upper` are None."""
    out = []
    for m in (metrics, metrics.get("asnorm") or {}):
        if m.get("eer") is None:
            continue
        pm = "" if m.get("eer_lower") is None or m.get("eer_upper") is None else f" ± {round((m['eer_upper'] - m['eer_lower']) / 2, 3)}"
        out.append(f" %EER: {round(m['eer'], 3)}{pm}, Min Cllr: {round(m['min_cllr'], 3)}, linkability: {round(m['linkability'], 3)}")
    return out


def main(argv=None):
    import argparse
    from .infer_helper import load_model
    ap = argparse.ArgumentParser(prog="asv-eval", description="ASV privacy metrics of a data directory (EER, min Cllr, linkability)")
    ap.add_argument("checkpoint", help="x-vector checkpoint (final.pt), or synthetic:xvector[?seed=N&speakers=K] / synthetic:xvector_resnet[?seed=N&speakers=K]")
    ap.add_argument("--enrolls-wav-scp", required=True)
    ap.add_argument("--trails-wav-scp", required=True)
    ap.add_argument("--enroll-utt2spk", required=True)
    ap.add_argument("--trials", required=True)
    ap.add_argument("--decode-output", required=True, help="directory for xvectors.npz, scores and metric.json")
    ap.add_argument("--no-as-norm", action="store_true", help="skip adaptive s-norm")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--eer-ci", type=int, default=0, metavar="M",
                    help="bootstrap replicates for the 95 %% interval of the EER (eer_lower / eer_upper; eer becomes the empirical EER); 0 = off")
    ap.add_argument("--eer-ci-seed", type=int, default=0, metavar="S", help="seed of the bootstrap draws")
    ap.add_argument("--report", action="store_true", help="also print the two lines of the reference's report step (raw, AS-norm)")
    ap.add_argument("--resnet-conv2d", choices=("f32", "f16x3"), default=None,
                    help="arithmetic of the 2-D convs of the ResNet extractor's blocks (its conv2d_precision); an error for the ECAPA model")
    ap.add_argument("--resnet-conv2d-ragged", choices=("f32", "f16x3"), default=None,
                    help="arithmetic of the same convs in the ragged batches of --batch-size above 1 (the ResNet extractor's "
                         "ragged_conv2d_precision, which --resnet-conv2d does not govern); an error for the ECAPA model")
    ap.add_argument("--batch-size", type=int, default=1, metavar="N",
                    help="utterances per extractor call: above 1 the model (ECAPA-TDNN or ResNet) extracts ragged batches of up to N utterances "
                         "of any lengths; 1 = one per call, the reference's way")
    ap.add_argument("--max-frames", type=int, default=65536, metavar="F",
                    help="most frames (10 ms each) in one ragged batch; the ResNet model's largest tensors take 10 KB per frame (671 MB at the "
                         "default, several live at once), the ECAPA-TDNN model's 6 KB")
    a = ap.parse_args(argv)
    if a.batch_size < 1 or a.max_frames < 1:
        ap.error("--batch-size and --max-frames take positive counts")
    if a.eer_ci < 0:
        ap.error("--eer-ci takes a count of replicates (0 = off)")
    model = load_model(a.checkpoint).to(a.device)
    if a.resnet_conv2d is not None:
        if not hasattr(model, "conv2d_precision"):
            ap.error("--resnet-conv2d: the loaded model is not the ResNet extractor (it has no 2-D convs)")
        model.conv2d_precision = a.resnet_conv2d
    if a.resnet_conv2d_ragged is not None:
        if not hasattr(model, "ragged_conv2d_precision"):
            ap.error("--resnet-conv2d-ragged: the loaded model is not the ResNet extractor (it has no 2-D convs)")
        model.ragged_conv2d_precision = a.resnet_conv2d_ragged
    ci = dict(m=a.eer_ci, ci=0.95, seed=a.eer_ci_seed) if a.eer_ci else None
    m = test_metrics(model, a.enrolls_wav_scp, a.trails_wav_scp, a.enroll_utt2spk, a.trials, a.decode_output, as_norm=not a.no_as_norm, eer_ci=ci,
                     **({} if a.batch_size == 1 else dict(batch_size=a.batch_size, max_frames=a.max_frames)))
    print(json.dumps({k: v for k, v in m.items() if k != "score"}))
    if a.report:
        print("\n".join(report_lines(m)))
