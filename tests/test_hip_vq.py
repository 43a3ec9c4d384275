"""The VQ kernel (`vq_kernel<NC, TIE>`, csrc/bottleneck.hip; reference VectorQuantizerEMA, chain/nn.py:424-459) against a float64
host model of the same operation: distances within an f32 rounding bound, the arg-min with first-minimum order, the quantised
output bit for bit, the near-tie count of the TIE variant, and the sizes it refuses.  Both template instances (48 and 64 codes,
padded codes included), D tails, T off the 64-frame block, the LDS opt-in past 64 KB and the LDS limit itself.
Needs a real MI355X: run with `-m gpu`."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT32_MAX = 2 ** 31 - 1

# (B, D, T, n_codes): every n_codes of {1, 2, 4, 47, 48, 49, 63, 64}, D of {256, 100, 7} (100 and 7: the tail loop d0 + 8 > D),
# T of {1, 63, 64, 65, 300, 4099}, B of {1, 3, 40}; (256, 64): 70 KB of LDS (hipFuncSetAttribute); D = 623 with 64 codes and D = 831
# with 48 are the largest the 160 KB of LDS hold ((NC D + NC + 1024) * 4 bytes)
CASES = [(2, 256, 300, 48), (1, 256, 1, 1), (3, 256, 65, 64), (3, 100, 63, 49), (1, 7, 64, 2), (40, 100, 4099, 63),
         (3, 7, 4099, 4), (1, 256, 64, 47), (2, 100, 1, 64), (40, 7, 65, 48), (3, 256, 300, 63), (1, 623, 300, 64),
         (2, 831, 130, 48), (1, 100, 4099, 1)]


def _ops():
    from satools_amd import _lib, ops
    return ops, _lib


def _inputs(B, D, T, n, seed):
    """z [B, D, T] N(0, 1), every 7th frame scaled by 1/100 (the zero rows of the padded codes would be nearest to those, were they
    not skipped); codebook rows = frames of z + N(0, 0.3^2): many frames have a second code close to the best"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, D, T, generator=g)
    z[:, :, ::7] *= 0.01
    frames = z.permute(0, 2, 1).reshape(-1, D)
    pick = torch.randint(0, frames.shape[0], (n,), generator=g)
    cb = (frames[pick] + 0.3 * torch.randn(n, D, generator=g)).contiguous()
    return z.contiguous(), cb


def _host(z, cb):
    """float64 expanded form of the distances (the reference's formula, chain/nn.py:424-432) -> (d64 [B, T, n], S [B, T, n]) with
    S = |z|^2 + |e|^2 + 2 |z| |e|, the sum of the magnitudes every term of the f32 evaluation is made of"""
    z64 = z.double().permute(0, 2, 1)
    e64 = cb.double()
    zz = (z64 * z64).sum(-1, keepdim=True)
    ee = (e64 * e64).sum(-1)
    d64 = (zz + ee) - 2.0 * (z64 @ e64.t())
    S = zz + ee + 2.0 * zz.sqrt() * ee.sqrt()
    return d64, S


def _dist_bound(S, D):
    """|d32 - d64| <= 2 * 2^-23 * sqrt(D) * S.  The kernel sums |z|^2, |e|^2 (separately rounded products) and z . e (an fma chain)
    in d order in f32, then two more roundings: worst case (D + 2) 2^-24 S; the rounding errors of a sequential sum of D terms
    behave like a random walk of standard deviation <= 2^-24 S sqrt(D) / 3, so the bound is 12 of those.  An f32 emulation of the
    kernel's order stays below 0.46 of it (D = 7 .. 623).  A wrong term — a code row dropped or mis-transposed in LDS, a skipped
    tail dimension, a padded code's zeros read as a real code — moves a distance by O(|z_d e_d|), orders of magnitude more."""
    return 2.0 * 2.0 ** -23 * math.sqrt(D) * S


def _vq(z, cb, tie=None):
    ops, _ = _ops()
    q, idx, dist = ops.vq(z.to(DEV), cb.to(DEV), want_dist=True, tie=tie)
    torch.cuda.synchronize()
    return q.cpu(), idx.cpu().long(), dist.cpu()


def _counts0(B):
    return torch.tensor([[0] * B, [INT32_MAX] * B, [-1] * B], dtype=torch.int32, device=DEV)


def _pair(cb):
    return torch.cdist(cb.double(), cb.double()).to(torch.float32).contiguous()


def _check_decisions(z, cb, q, idx, dist):
    B, D, T = z.shape
    n = cb.shape[0]
    assert dist.shape == (B, T, n) and idx.shape == (B, T) and q.shape == z.shape
    d64, S = _host(z, cb)
    err = (dist.double() - d64).abs()
    bound = _dist_bound(S, D)
    assert (err <= bound).all(), f"distance error {float((err / bound).max()):.2f} x the bound"
    # the arg-min of the kernel's own distances, first minimum in code order (torch.argmin): the merge of the four code groups
    assert torch.equal(idx, torch.argmin(dist, dim=-1))
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    # against float64: the f64 best wherever its margin exceeds what the two distances' errors can swap
    best64 = torch.argmin(d64, dim=-1)
    srt = torch.sort(d64, dim=-1)[0]
    margin = srt[..., 1] - srt[..., 0] if n > 1 else torch.full_like(srt[..., 0], math.inf)
    emax = err.max(dim=-1)[0]
    sure = margin > 2 * emax
    assert torch.equal(idx[sure], best64[sure])
    # elsewhere one of the codes within that reach of the f64 best (with random codes: one of the two best)
    d_at = torch.gather(d64, -1, idx.unsqueeze(-1)).squeeze(-1)
    assert (d_at - srt[..., 0] <= 2 * emax).all()
    # q = `inputs + (quantized - inputs)` (chain/nn.py:459) with the kernel's indices, bit for bit
    zt = z.permute(0, 2, 1)
    ref_q = (zt + (cb[idx] - zt)).permute(0, 2, 1)
    assert torch.equal(q, ref_q)
    return int((~sure).sum())


def _host_xx(z):
    """the kernel's f32 |z_t|^2: separately rounded squares added in d order ([B, T] f32, bit-exact)"""
    zt = z.permute(0, 2, 1).contiguous().numpy()
    xx = np.zeros(zt.shape[:2], np.float32)
    for d in range(zt.shape[2]):
        xx = xx + zt[:, :, d] * zt[:, :, d]
    return torch.from_numpy(xx)


def _host_tie(dist, z, pair, scale):
    """the TIE rule on the kernel's own distances: best and runner-up in first-minimum order, flagged <=> !(gap > scale sqrt(|z|^2)
    pair[best, runner-up]), all in f32 as the kernel evaluates it -> (flagged [B, T] bool, ambiguous [B, T] bool: within 1e-6
    relative of the threshold, where sqrtf's last bit could decide)"""
    B, T, n = dist.shape
    if n < 2:
        return torch.zeros(B, T, dtype=torch.bool), torch.zeros(B, T, dtype=torch.bool)
    best = torch.argmin(dist, dim=-1)
    rest = dist.clone()
    rest.scatter_(-1, best.unsqueeze(-1), math.inf)
    second = torch.argmin(rest, dim=-1)
    gap = torch.gather(dist, -1, second.unsqueeze(-1)).squeeze(-1) - torch.gather(dist, -1, best.unsqueeze(-1)).squeeze(-1)
    th = (torch.tensor(scale, dtype=torch.float32) * _host_xx(z).sqrt()) * pair[best, second]
    flagged = ~(gap > th)
    amb = (gap - th).abs().double() <= 1e-6 * th.double().abs()
    return flagged, amb & (th > 0)


def _check_counts(counts, flagged, amb):
    """tie_count [3, B] (count | first | last flagged frame) against the host's flags, per utterance"""
    counts = counts.cpu().long()
    for b in range(flagged.shape[0]):
        sure = torch.nonzero(flagged[b] & ~amb[b]).flatten()
        maybe = torch.nonzero(flagged[b] | amb[b]).flatten()
        c, first, last = (int(v) for v in counts[:, b])
        if maybe.numel() == 0:
            assert (c, first, last) == (0, INT32_MAX, -1), (b, c, first, last)
        elif maybe.numel() == sure.numel():
            assert (c, first, last) == (sure.numel(), int(sure[0]), int(sure[-1])), (b, c, first, last, sure.tolist()[:8])
        else:
            assert sure.numel() <= c <= maybe.numel(), (b, c, sure.numel(), maybe.numel())
            if c:
                assert first in maybe.tolist() and last in maybe.tolist() and first <= last
                if sure.numel():
                    assert first <= int(sure[0]) and last >= int(sure[-1])


@pytest.mark.parametrize("B,D,T,n", CASES, ids=lambda v: str(v))
def test_vq_against_float64(B, D, T, n):
    z, cb = _inputs(B, D, T, n, seed=B * 7919 + D * 31 + T + n)
    q, idx, dist = _vq(z, cb)
    close = _check_decisions(z, cb, q, idx, dist)
    print(f"vq B={B} D={D} T={T} n={n}: {close} of {B * T} frames inside the f64 margin rule")


@pytest.mark.parametrize("B,D,T,n", CASES, ids=lambda v: str(v))
def test_vq_tie_variant_counts_the_near_ties(B, D, T, n):
    """sat_vq_argmin_gather_tie_f32: the plain entry's bits for idx, q and dist, and tie_count [3, B] = the host's recomputation of the
    rule from the kernel's own distances — at a window that flags about a fifth of the frames, at 0 (exact equal distances only) and
    at a window so wide that every live frame is flagged (and no dead lane of the last 64-frame block)"""
    z, cb = _inputs(B, D, T, n, seed=B * 7919 + D * 31 + T + n)
    q, idx, dist = _vq(z, cb)
    pair = _pair(cb)
    pd = pair.to(DEV)
    # a window at the 20th percentile of the frames' gap / (|z| pair) ratio (any positive value for a single code)
    if n > 1:
        best = torch.argmin(dist, dim=-1)
        rest = dist.clone().scatter_(-1, best.unsqueeze(-1), math.inf)
        second = torch.argmin(rest, dim=-1)
        ratio = (rest.min(dim=-1)[0] - dist.min(dim=-1)[0]).double() / (_host_xx(z).double().sqrt() * pair[best, second].double())
        mid = float(torch.quantile(ratio.flatten()[:1 << 20], 0.2))
    else:
        mid = 1.0
    for scale in (mid, 0.0, 1e30):
        counts = _counts0(B)
        qt, it, dt = _vq(z, cb, tie=(pd, scale, counts))
        assert torch.equal(qt, q) and torch.equal(it, idx) and torch.equal(dt, dist)
        flagged, amb = _host_tie(dist, z, pair, scale)
        _check_counts(counts, flagged, amb)
        c = counts.cpu().long()
        if scale == 1e30:
            if n >= 2:
                assert c[0].tolist() == [T] * B and c[1].tolist() == [0] * B and c[2].tolist() == [T - 1] * B, c
            else:                                   # no runner-up: nothing is a near-tie
                assert c[0].tolist() == [0] * B and c[1].tolist() == [INT32_MAX] * B and c[2].tolist() == [-1] * B, c
        if scale == 0.0 and n >= 2:                 # window 0: the frames whose two best f32 distances are equal, and only those
            srt = torch.sort(dist, dim=-1)[0]
            assert int(c[0].sum()) == int((srt[..., 0] == srt[..., 1]).sum())
        print(f"vq tie B={B} D={D} T={T} n={n} scale={scale:.3g}: {int(c[0].sum())} frames flagged ({int(amb.sum())} at the threshold)")


def _integer_codebook(n, D, seed, lo=-4, hi=5, even=False):
    g = torch.Generator().manual_seed(seed)
    cb = torch.randint(lo, hi, (n, D), generator=g).float()
    return cb * 2 if even else cb


@pytest.mark.parametrize("n,dups", [(48, [(3, 5)]), (48, [(5, 40)]), (64, [(11, 60)]), (48, [(7, 20, 33, 46)]),
                                    (64, [(15, 16), (31, 47, 63)]), (49, [(0, 48)]), (64, [(20, 45)])],
                         ids=lambda v: str(v))
def test_vq_first_minimum_on_duplicated_codes(n, dups):
    """small-integer codebooks and frames: every f32 distance is exact.  Rows duplicated inside one wave's code group (12 codes per
    group at NC = 48, 16 at NC = 64) and across groups; frames at (or near) a duplicated row: the index is the LOWEST of the
    duplicates, as torch.argmin gives — both in the group-local scan and in the merge of the four groups.  The TIE variant at
    window 0 flags exactly the frames whose two best distances are equal."""
    B, D, T = 3, 100, 130
    cb = _integer_codebook(n, D, seed=n + len(dups))
    for grp in dups:
        for r in grp[1:]:
            cb[r] = cb[grp[0]]
    g = torch.Generator().manual_seed(7)
    zt = torch.randint(-4, 5, (B, T, D), generator=g).float()
    targets = [r for grp in dups for r in grp]
    for t in range(T):
        for b in range(B):
            if (t + b) % 3:                          # two thirds of the frames at a duplicated row, +-1 on a few components
                zt[b, t] = cb[targets[(t + b) % len(targets)]] + (torch.randint(-1, 2, (D,), generator=g) * (torch.rand(D, generator=g) < 0.1))
    z = zt.permute(0, 2, 1).contiguous()
    q, idx, dist = _vq(z, cb)
    d64, _ = _host(z, cb)
    assert torch.equal(dist.double(), d64)                 # integers: exact in f32
    assert torch.equal(idx, torch.argmin(d64, dim=-1))     # first minimum
    hit = torch.tensor([[int(idx[b, t]) in [grp[0] for grp in dups] for t in range(T)] for b in range(B)])
    assert int(hit.sum()) >= B * T // 2                   # the duplicated rows are where most frames land: the lowest of each group
    for grp in dups:
        assert not any(int(v) in grp[1:] for v in idx.flatten())
    counts = _counts0(B)
    qt, it, dt = _vq(z, cb, tie=(_pair(cb).to(DEV), 0.0, counts))
    assert torch.equal(qt, q) and torch.equal(it, idx) and torch.equal(dt, dist)
    srt = torch.sort(d64, dim=-1)[0]
    eq = srt[..., 0] == srt[..., 1]
    _check_counts(counts, eq, torch.zeros_like(eq))
    assert int(counts[0].sum()) == int(eq.sum()) > 0


@pytest.mark.parametrize("n,pairs", [(48, [(3, 5), (5, 40), (0, 47), (11, 12), (20, 45)]),
                                     (64, [(11, 60), (15, 16), (47, 48), (0, 63), (30, 33)]),
                                     (49, [(1, 48), (12, 47)]), (4, [(0, 3), (1, 2)])], ids=lambda v: str(v))
def test_vq_first_minimum_between_equidistant_codes(n, pairs):
    """frames z = (e_a + e_b) / 2 of two DISTINCT codes with even integer entries: exactly equidistant in f32, and nearer to those two
    than to any other code; the index is the lower one, in one group and across groups.  The TIE variant at window 0 flags these
    frames and no other."""
    B, D, T = 2, 256, 65
    cb = _integer_codebook(n, D, seed=100 + n, even=True)
    g = torch.Generator().manual_seed(11)
    zt = torch.randint(-8, 9, (B, T, D), generator=g).float()
    mids = torch.zeros(B, T, dtype=torch.bool)
    for t in range(0, T, 2):
        for b in range(B):
            a, c = pairs[(t // 2 + b) % len(pairs)]
            zt[b, t] = (cb[a] + cb[c]) / 2
            mids[b, t] = True
    z = zt.permute(0, 2, 1).contiguous()
    q, idx, dist = _vq(z, cb)
    d64, _ = _host(z, cb)
    assert torch.equal(dist.double(), d64)
    srt = torch.sort(d64, dim=-1)[0]
    eq = srt[..., 0] == srt[..., 1]
    assert eq[mids].all()                                   # the constructed frames are exact two-way ties of the best distance
    assert torch.equal(idx, torch.argmin(d64, dim=-1))
    for t in range(0, T, 2):
        for b in range(B):
            assert int(idx[b, t]) == min(pairs[(t // 2 + b) % len(pairs)]), (b, t)
    counts = _counts0(B)
    qt, it, dt = _vq(z, cb, tie=(_pair(cb).to(DEV), 0.0, counts))
    assert torch.equal(qt, q) and torch.equal(it, idx) and torch.equal(dt, dist)
    _check_counts(counts, eq, torch.zeros_like(eq))


def test_vq_refuses_sizes_past_its_instances_and_the_lds():
    """n_codes = 65 (VQ_MAX_CODES = 64) and a codebook that does not fit the 160 KB of LDS ((NC D + NC + 1024) * 4 bytes: D = 624
    with 64 codes, D = 832 with 48) raise SatError before any launch; a valid call on the same stream still runs afterwards"""
    ops, _lib = _ops()
    for (D, n) in ((16, 65), (624, 64), (832, 48), (832, 2)):
        z = torch.randn(1, D, 64).to(DEV)
        cb = torch.randn(n, D).to(DEV)
        with pytest.raises(_lib.SatError):
            ops.vq(z, cb, want_dist=True)
        with pytest.raises(_lib.SatError):
            ops.vq(z, cb, want_dist=True, tie=(torch.zeros(n, n, device=DEV), 1.0, _counts0(1)))
    torch.cuda.synchronize()
    z, cb = _inputs(1, 623, 64, 64, seed=5)
    q, idx, dist = _vq(z, cb)
    _check_decisions(z, cb, q, idx, dist)
