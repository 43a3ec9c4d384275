"""The tiled VQ kernel (`vq_tiled_kernel<TIE, PF>`, csrc/vq_tiled.hip; reference VectorQuantizerEMA, chain/nn.py:424-459) — the
codebook walked in 64-code tiles through LDS, for codebooks that do not fit it whole (the 256-code tag) — against the float64 host
model and the checks of tests/test_hip_vq.py: distances within the f32 rounding bound, the arg-min with first-minimum order, q bit
for bit, the near-tie counts of the TIE variant; exact two-way ties whose codes lie in DIFFERENT tiles; for at most 64 codes the
bits of the existing kernel; and the sizes it refuses.
Needs a real MI355X: run with `-m gpu`."""
import math

import pytest
import torch

from test_hip_vq import (CASES as VQ_CASES, DEV, INT32_MAX, _check_counts, _check_decisions, _counts0, _host, _host_tie, _host_xx, _inputs,
                         _integer_codebook, _ops, _pair)

pytestmark = pytest.mark.gpu

# (B, D, T, n_codes): n_codes of {1, 48, 64, 65, 100, 128, 129, 255, 256, 257, 1024} (tile edges, ragged last tiles), D of {256, 100, 7},
# T of {1, 63, 64, 65, 300, 4099}, B of {1, 3, 40}; D = 300 and 623 take the instance without the register prefetch (a tile of more
# than 256 x 64 values), 623 being the largest D whose tile fits the 160 KB of LDS ((64 D + 1088) * 4 bytes)
CASES = [(2, 256, 300, 256), (1, 256, 1, 1), (3, 256, 65, 64), (3, 100, 63, 65), (1, 7, 64, 100), (40, 100, 300, 128),
         (3, 7, 4099, 129), (1, 256, 64, 255), (40, 256, 65, 257), (3, 256, 300, 1024), (1, 100, 4099, 48), (40, 7, 1, 256),
         (3, 100, 65, 1024), (1, 7, 63, 257), (1, 623, 130, 130), (2, 300, 70, 65)]


def _vqt(z, cb, tie=None):
    ops, _ = _ops()
    q, idx, dist = ops.vq_tiled(z.to(DEV), cb.to(DEV), want_dist=True, tie=tie)
    torch.cuda.synchronize()
    return q.cpu(), idx.cpu().long(), dist.cpu()


@pytest.mark.parametrize("B,D,T,n", CASES, ids=lambda v: str(v))
def test_vq_tiled_against_float64(B, D, T, n):
    z, cb = _inputs(B, D, T, n, seed=B * 7919 + D * 31 + T + n)
    q, idx, dist = _vqt(z, cb)
    close = _check_decisions(z, cb, q, idx, dist)
    print(f"vq_tiled B={B} D={D} T={T} n={n}: {close} of {B * T} frames inside the f64 margin rule")
    # without the distances asked for: the same decisions
    ops, _ = _ops()
    q2, idx2, none = ops.vq_tiled(z.to(DEV), cb.to(DEV))
    assert none is None and torch.equal(q2.cpu(), q) and torch.equal(idx2.cpu().long(), idx)


@pytest.mark.parametrize("B,D,T,n", CASES, ids=lambda v: str(v))
def test_vq_tiled_tie_variant_counts_the_near_ties(B, D, T, n):
    """sat_vq_argmin_gather_tiled_tie_f32: the plain entry's bits for idx, q and dist, and tie_count [3, B] = the host's recomputation
    of the rule from the kernel's own distances, at a window that flags about a fifth of the frames, at 0 and at one that flags all"""
    z, cb = _inputs(B, D, T, n, seed=B * 7919 + D * 31 + T + n)
    q, idx, dist = _vqt(z, cb)
    pair = _pair(cb)
    pd = pair.to(DEV)
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
        qt, it, dt = _vqt(z, cb, tie=(pd, scale, counts))
        assert torch.equal(qt, q) and torch.equal(it, idx) and torch.equal(dt, dist)
        flagged, amb = _host_tie(dist, z, pair, scale)
        _check_counts(counts, flagged, amb)
        c = counts.cpu().long()
        if scale == 1e30:
            if n >= 2:
                assert c[0].tolist() == [T] * B and c[1].tolist() == [0] * B and c[2].tolist() == [T - 1] * B, c
            else:
                assert c[0].tolist() == [0] * B and c[1].tolist() == [INT32_MAX] * B and c[2].tolist() == [-1] * B, c
        if scale == 0.0 and n >= 2:
            srt = torch.sort(dist, dim=-1)[0]
            assert int(c[0].sum()) == int((srt[..., 0] == srt[..., 1]).sum())
        print(f"vq_tiled tie B={B} D={D} T={T} n={n} scale={scale:.3g}: {int(c[0].sum())} frames flagged ({int(amb.sum())} at the threshold)")


@pytest.mark.parametrize("n,dups", [(256, [(5, 200)]), (130, [(63, 64, 129)]), (1024, [(15, 16), (31, 700, 1023)]), (257, [(0, 256)]),
                                    (100, [(20, 45), (47, 80)])], ids=lambda v: str(v))
def test_vq_tiled_first_minimum_on_duplicated_codes(n, dups):
    """small-integer codebooks and frames (every f32 distance exact), rows duplicated across tiles and across the waves' code groups:
    the index is the LOWEST of the duplicates, and the TIE variant at window 0 flags exactly the frames whose two best are equal"""
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
            if (t + b) % 3:
                zt[b, t] = cb[targets[(t + b) % len(targets)]] + (torch.randint(-1, 2, (D,), generator=g) * (torch.rand(D, generator=g) < 0.1))
    z = zt.permute(0, 2, 1).contiguous()
    q, idx, dist = _vqt(z, cb)
    d64, _ = _host(z, cb)
    assert torch.equal(dist.double(), d64)
    assert torch.equal(idx, torch.argmin(d64, dim=-1))
    for grp in dups:
        assert not any(int(v) in grp[1:] for v in idx.flatten())
    counts = _counts0(B)
    qt, it, dt = _vqt(z, cb, tie=(_pair(cb).to(DEV), 0.0, counts))
    assert torch.equal(qt, q) and torch.equal(it, idx) and torch.equal(dt, dist)
    srt = torch.sort(d64, dim=-1)[0]
    eq = srt[..., 0] == srt[..., 1]
    _check_counts(counts, eq, torch.zeros_like(eq))
    assert int(counts[0].sum()) == int(eq.sum()) > 0


@pytest.mark.parametrize("n,pairs", [(256, [(3, 200), (63, 64), (70, 129), (0, 255), (100, 228)]),
                                     (1024, [(11, 1000), (127, 128), (512, 1023), (0, 64)]),
                                     (65, [(1, 64), (63, 64)]), (130, [(5, 129), (64, 128)])], ids=lambda v: str(v))
def test_vq_tiled_first_minimum_between_equidistant_codes_of_different_tiles(n, pairs):
    """frames z = (e_a + e_b) / 2 of two DISTINCT codes with even integer entries that lie in different 64-code tiles: exactly
    equidistant in f32 and nearer to those two than to any other code; the lower code wins, and with tie_scale = 0 exactly those
    frames are counted"""
    assert all(a // 64 != c // 64 for a, c in pairs)
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
    q, idx, dist = _vqt(z, cb)
    d64, _ = _host(z, cb)
    assert torch.equal(dist.double(), d64)
    srt = torch.sort(d64, dim=-1)[0]
    eq = srt[..., 0] == srt[..., 1]
    assert eq[mids].all()
    assert torch.equal(idx, torch.argmin(d64, dim=-1))
    for t in range(0, T, 2):
        for b in range(B):
            assert int(idx[b, t]) == min(pairs[(t // 2 + b) % len(pairs)]), (b, t)
    counts = _counts0(B)
    qt, it, dt = _vqt(z, cb, tie=(_pair(cb).to(DEV), 0.0, counts))
    assert torch.equal(qt, q) and torch.equal(it, idx) and torch.equal(dt, dist)
    _check_counts(counts, eq, torch.zeros_like(eq))
    assert int(counts[0].sum()) == int(eq.sum()) and int(eq.sum()) >= int(mids.sum())


@pytest.mark.parametrize("B,D,T,n", [c for c in VQ_CASES if c[1] <= 623], ids=lambda v: str(v))
def test_vq_tiled_has_the_bits_of_the_lds_kernel_up_to_64_codes(B, D, T, n):
    """the twin: same formula, same order of every chain, same first-minimum rule — dist, idx, q and tie_count of the tiled entry
    points equal those of sat_vq_argmin_gather_f32 / _tie_f32 bit for bit on the cases of tests/test_hip_vq.py"""
    ops, _ = _ops()
    z, cb = _inputs(B, D, T, n, seed=B * 7919 + D * 31 + T + n)
    zd, cd = z.to(DEV), cb.to(DEV)
    q0, i0, d0 = ops.vq(zd, cd, want_dist=True)
    q1, i1, d1 = ops.vq_tiled(zd, cd, want_dist=True)
    assert torch.equal(d0, d1) and torch.equal(i0, i1) and torch.equal(q0, q1)
    pd = _pair(cb).to(DEV)
    ratio = 1.0
    if n > 1:
        srt = torch.sort(d0.cpu(), dim=-1)[0]
        ratio = float(torch.quantile(((srt[..., 1] - srt[..., 0]).double() / _host_xx(z).double().sqrt().clamp_min(1e-30)).flatten()[:1 << 20], 0.2))
    for scale in (ratio / float(pd.max().clamp_min(1e-30)), ratio / float(pd.mean().clamp_min(1e-30)), 0.0, 1e30):
        c0, c1 = _counts0(B), _counts0(B)
        q0, i0, d0 = ops.vq(zd, cd, want_dist=True, tie=(pd, scale, c0))
        q1, i1, d1 = ops.vq_tiled(zd, cd, want_dist=True, tie=(pd, scale, c1))
        torch.cuda.synchronize()
        assert torch.equal(d0, d1) and torch.equal(i0, i1) and torch.equal(q0, q1)
        assert torch.equal(c0, c1), (scale, c0.tolist(), c1.tolist())
        print(f"twin B={B} D={D} T={T} n={n} scale={scale:.3g}: {int(c0[0].sum())} frames flagged by both")


def test_vq_tiled_refuses_sizes_past_its_limits():
    """n_codes = 1025 and a D whose 64-code tile does not fit the 160 KB of LDS ((64 D + 1088) * 4 bytes: D = 624) raise SatError on
    the host, before any launch; a valid call on the same stream runs afterwards"""
    ops, _lib = _ops()
    for (D, n) in ((16, 1025), (624, 64), (624, 256), (1000, 2)):
        z = torch.randn(1, D, 64).to(DEV)
        cb = torch.randn(n, D).to(DEV)
        with pytest.raises(_lib.SatError):
            ops.vq_tiled(z, cb, want_dist=True)
        with pytest.raises(_lib.SatError):
            ops.vq_tiled(z, cb, want_dist=True, tie=(torch.zeros(n, n, device=DEV), 1.0, _counts0(1)))
    z = torch.randn(1, 16, 64).to(DEV)
    cb = torch.randn(70, 16).to(DEV)
    with pytest.raises(_lib.SatError):           # a pair table of the wrong shape
        ops.vq_tiled(z, cb, tie=(torch.zeros(64, 64, device=DEV), 1.0, _counts0(1)))
    torch.cuda.synchronize()
    z, cb = _inputs(1, 623, 64, 256, seed=5)
    q, idx, dist = _vqt(z, cb)
    _check_decisions(z, cb, q, idx, dist)
