"""Float64 restatement of the WIDE frame means of YAAPT's time-domain stage (csrc/yaapt_long/yaapt_long.hip: frames that overlap more
than their predecessor), for tests; the companion of tests/ref64_yaapt.py, whose conventions (U, FLOOR, `_ratio`, the judges' result
dicts) and whose NCCF references (`nccf_phi`, `nccf_pick`, `nccf_merit`, `judge_nccf`) are used unchanged.

The quantity.  With n = tda_len, J = frame_jump, D = ceil(n / J) - 1, sample j of frame k reaches crs_corr as
    v = x[k J + j];   for i = D .. 1:  if k - i >= 0 and j < n - i J:  v = fl32(v - mean[k - i])
    mean[k] = mean_j(v);   d[j] = fl32(v - mean[k])
Every frame is checked ON ITS OWN from the means the implementation itself produced for the D frames before it, so an error does not travel
down the recurrence (as `ref64_yaapt.frame_means` does for D = 1).

The bound.  A sample of segment s (j in n - (s + 1) J .. n - s J) passes through s rounded subtractions before it is summed: each costs
U |value after it| (the partial values are formed here in float64, one after the other, and their magnitudes summed: `subs`).  The sum
itself collects `WideRoundings.head(n, J)` roundings on the terms with j < n - J (the part on the recurrence: the implementation's head)
and `WideRoundings.tail(n, J)` on the others, read off the summation order of the code under test; joining the two partial sums and the
division are the 2 |S| of `ref64_yaapt.frame_means`, the float32 store its U |S / n|.  Nothing is fitted to an implementation's output."""
import math

import numpy as np

import ref64_yaapt as r64
from ref64_yaapt import FLOOR, U, _f64, _ratio


class WideRoundings:
    """head(n, hop), tail(n, hop): the roundings a term of the head (j < n - hop) and of the tail collects in the frame's sum"""

    def __init__(self, head, tail):
        self.head, self.tail = head, tail


# a float32 implementation that sums a frame in any order (torch.mean of the float32 oracle): at most n - 1 additions on any term
ANY_ORDER = WideRoundings(head=lambda n, hop: n, tail=lambda n, hop: n)


def depth(plan):
    return math.ceil(plan.tda_len / plan.frame_jump) - 1


def frame_means_wide(x, prev_means, plan, W):
    """x float32 [>= (T - 1) hop + n]; prev_means [T] float32 = the implementation's own means (frame k uses prev_means[k - D .. k - 1] as
    given) -> (mean [T], bound [T])"""
    T, n, hop = plan.tda_nframes, plan.tda_len, plan.frame_jump
    D, ov = depth(plan), plan.tda_len - plan.frame_jump
    idx = (np.arange(T) * hop)[:, None] + np.arange(n)[None, :]
    v = _f64(x)[idx]
    pm = _f64(prev_means)
    subs = np.zeros(T)
    for i in range(D, 0, -1):                              # the oldest frame first: frame k - i covers the first n - i hop samples of frame k
        w = n - i * hop
        if T > i:
            v[i:, :w] -= pm[:T - i, None]
            subs[i:] += np.abs(v[i:, :w]).sum(1)
    head, tail = v[:, :ov], v[:, ov:]
    S = head.sum(1) + tail.sum(1)
    bound = U * (subs + W.head(n, hop) * np.abs(head).sum(1) + W.tail(n, hop) * np.abs(tail).sum(1) + 2 * np.abs(S)) / n
    return S / n, bound + U * np.abs(S / n) + FLOOR


def demeaned_frame_wide(x, k, means, plan):
    """the float32 frame crs_corr sees: up to D + 1 correctly rounded float32 subtractions per sample, reproduced here bit for bit"""
    n, hop = plan.tda_len, plan.frame_jump
    v = np.asarray(x[k * hop:k * hop + n], dtype=np.float32).copy()
    for i in range(depth(plan), 0, -1):
        if k - i >= 0:
            w = n - i * hop
            v[:w] = v[:w] - np.float32(means[k - i])
    return v - np.float32(means[k])


def judge_fmean_wide(x, fmean, plan, W):
    want, bound = frame_means_wide(x, fmean, plan, W)
    return dict(ratio=_ratio(np.asarray(fmean)[:plan.tda_nframes], want, bound))


def judge_nccf_wide(x, fmean, spec_pitch, pitch_std, tp, tm, plan, R):
    """`ref64_yaapt.judge_nccf` itself, on frames rebuilt with `demeaned_frame_wide`: the lag window, phi and its bound, the pick and the
    merit are that module's, statement for statement"""
    keep, r64.demeaned_frame = r64.demeaned_frame, demeaned_frame_wide
    try:
        return r64.judge_nccf(x, fmean, spec_pitch, pitch_std, tp, tm, plan, R)
    finally:
        r64.demeaned_frame = keep
