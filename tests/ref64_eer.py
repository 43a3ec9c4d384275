"""The bootstrap of the empirical EER restated for the tests, apart from the product code (satools_amd.asv_eval, ops.eer_bootstrap,
csrc/stats/eer_bootstrap.hip): Philox4x32-10 in numpy uint64, the draws of a replicate, a replicate's two counts by histogram and prefix
sum over ALL K + 1 thresholds (the kernel bisects; asv_eval searches sorted arrays), and the definition itself, threshold by threshold in
Python integers, for small lists.  Everything here is integers or exact fractions: the comparisons that use it demand equality."""
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4] and key (k0, k1) of 32-bit words -> [..., 4] output words (uint64 arrays holding 32-bit values)"""
    c = np.asarray(counter, dtype=np.uint64)
    assert c.shape[-1] == 4 and int(c.max(initial=0)) < 2 ** 32
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]), int(key[1])
    assert 0 <= k0 < 2 ** 32 and 0 <= k1 < 2 ** 32
    for _ in range(10):
        p0 = np.uint64(M0) * c0                # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> SH) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> SH) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1)


def words(n, r, s, seed, count=None):
    """the first `count` (default: all n) random words of stream s of replicate r: word j = output word j & 3 at the counter (j >> 2, r, s, 0)"""
    count = n if count is None else min(count, n)
    q = np.arange((count + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q, np.full_like(q, r), np.full_like(q, s), np.zeros_like(q)], axis=-1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:count]


def draws(n, r, s, seed, count=None):
    """the n indices of 0 .. n - 1 replicate r draws from stream s: (word * n) >> 32 -> int64 [n] (or the first `count` of them)"""
    assert 1 <= n < 2 ** 32
    return ((words(n, r, s, seed, count) * np.uint64(n)) >> SH).astype(np.int64)


def eer_counts(tar_sorted, non_sorted, idx_t, idx_n):
    """the sets resampled as tar_sorted[idx_t], non_sorted[idx_n] -> (miss(k*), fa(k* - 1)) as Python integers.  The thresholds are the K
    distinct values of the ORIGINAL sets and +inf; every resampled score is counted into the histogram bin of its value, the exclusive
    prefix sums are miss(k) and n_non - fa(k) at all K + 1 thresholds, and k* is read off the whole predicate vector"""
    tar_sorted, non_sorted = np.asarray(tar_sorted, dtype=np.float64), np.asarray(non_sorted, dtype=np.float64)
    v = np.unique(np.concatenate([tar_sorted, non_sorted]))
    K = len(v)
    n_tar, n_non = len(idx_t), len(idx_n)
    assert n_tar == len(tar_sorted) and n_non == len(non_sorted)
    bin_t, bin_n = np.searchsorted(v, tar_sorted), np.searchsorted(v, non_sorted)
    assert np.array_equal(v[bin_t], tar_sorted) and np.array_equal(v[bin_n], non_sorted)
    miss = np.concatenate([[0], np.cumsum(np.bincount(bin_t[idx_t], minlength=K))]).astype(np.int64)
    fa = n_non - np.concatenate([[0], np.cumsum(np.bincount(bin_n[idx_n], minlength=K))]).astype(np.int64)
    assert n_tar * n_non < 2 ** 62
    pred = miss * n_non >= fa * n_tar
    assert not pred[0] and pred[K] and np.all(pred[1:] >= pred[:-1])
    k = int(np.argmax(pred))
    return int(miss[k]), int(fa[k - 1])


def replicate(tar_sorted, non_sorted, r, seed):
    """replicate r of the bootstrap -> (miss(k*), fa(k* - 1))"""
    return eer_counts(tar_sorted, non_sorted, draws(len(tar_sorted), r, 0, seed), draws(len(non_sorted), r, 1, seed))


def replicates(tar_sorted, non_sorted, first, m, seed):
    """-> (miss_at [m], fa_before [m]) int64 of the replicates first .. first + m - 1"""
    out = np.array([replicate(tar_sorted, non_sorted, first + i, seed) for i in range(m)], dtype=np.int64).reshape(m, 2)
    return out[:, 0].copy(), out[:, 1].copy()


def brute_eer(tar, non, weights=None):
    """the definition, threshold by threshold, in Python integers and exact fractions -> (eer as a float, miss(k*), fa(k* - 1)).
    weights = (multiplicity of every target, multiplicity of every non-target): the resampled sets; the thresholds stay those of the lists
    as given.  Also checks that the result is min_t max(P_miss(t), P_fa(t)).  For lists of up to about 20 values."""
    tar, non = [float(x) for x in tar], [float(x) for x in non]
    wt, wn = ([1] * len(tar), [1] * len(non)) if weights is None else ([int(w) for w in weights[0]], [int(w) for w in weights[1]])
    n_tar, n_non = sum(wt), sum(wn)
    assert n_tar > 0 and n_non > 0
    ts = sorted(set(tar) | set(non)) + [float("inf")]
    miss = [sum(w for x, w in zip(tar, wt) if x < t) for t in ts]
    fa = [sum(w for x, w in zip(non, wn) if x >= t) for t in ts]
    assert miss[0] == 0 and fa[0] == n_non and fa[-1] == 0 and miss[-1] == n_tar
    assert all(a <= b for a, b in zip(miss, miss[1:])) and all(a >= b for a, b in zip(fa, fa[1:]))
    k = next(i for i in range(len(ts)) if miss[i] * n_non >= fa[i] * n_tar)
    assert 1 <= k <= len(ts) - 1
    eer = min(Fraction(miss[k], n_tar), Fraction(fa[k - 1], n_non))
    assert eer == min(max(Fraction(a, n_tar), Fraction(b, n_non)) for a, b in zip(miss, fa))
    return min(miss[k] / n_tar, fa[k - 1] / n_non), miss[k], fa[k - 1]
