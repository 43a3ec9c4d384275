"""The properties tests/w2v2_lengths.py declares for its entries, from `TdnnfWav2vec2VqNet._fe_lens` and the oracle's frame
arithmetic, and the consistency of tests/golden/fx_w2v2_lengths.npz with the catalogue.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import w2v2_lengths as WL
from oracle import wav2vec2 as ow
from satools_amd.wav2vec2 import CONV_LAYERS, TdnnfWav2vec2VqNet, frames_out

fe_lens = TdnnfWav2vec2VqNet._fe_lens


def oracle_layer_frames(n):
    """the frame count after each conv layer of the oracle's feature extractor, from torch's own conv shape arithmetic (meta
    tensors: no data); None where torch refuses the input as too short"""
    x = torch.empty(1, 1, n, device="meta")
    lens = []
    for _, k, s in ow.CONV_LAYERS:
        if x.shape[2] < k:
            return None
        x = F.conv1d(x, torch.empty(1, 1, k, device="meta"), stride=s)
        lens.append(x.shape[2])
    return lens


def test_fe_lens_equal_the_oracles_layer_frame_counts():
    assert CONV_LAYERS == ow.CONV_LAYERS
    for n in list(range(400, 1361)) + [e.n for e in WL.ENTRIES if e.T] + [WL.BY_NAME[name].n for name, _ in WL.CONVERT]:
        lens = fe_lens(n)
        assert lens == oracle_layer_frames(n), n
        assert lens[-1] == ow.frames_out(n) == frames_out(n) == WL.frames(n), n
    for n in range(0, 400):                     # below one final frame: the product refuses on L6 < 1, torch on a layer shorter than its kernel
        assert fe_lens(n)[-1] < 1 and oracle_layer_frames(n) is None, n


def test_parity_set_has_all_64_patterns_at_three_frames():
    assert len(WL.PARITY) == WL.PARITY_COUNT == 64
    pats = set()
    for k, e in enumerate(WL.PARITY):
        assert e.n == WL.PARITY_N0 + WL.PARITY_STEP * k and e.B == 1
        lens = fe_lens(e.n)
        assert lens[-1] == e.T == WL.PARITY_T == 3
        pats.add(WL.parity_pattern(lens))
    assert len(pats) == 64
    # what the tests before this catalogue ran end to end: all odd, and 100000 with an even L5 alone
    old = {WL.parity_pattern(fe_lens(n)) for n in (16000, 17600, 19200, 32000, 80000, 100000, 320000, 560000)}
    assert old == {(1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 1, 0)}


def test_every_named_frame_count_edge():
    T = {e.name: fe_lens(e.n)[-1] for e in WL.ENTRIES}
    assert [T[e.name] for e in WL.T_EDGES] == [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257]
    assert [e.n for e in WL.T_EDGES] == [400, 720, 1040, 10000, 10320, 10640, 20240, 20560, 20880, 81680, 82000, 82320]
    assert all(e.T == T[e.name] for e in WL.ENTRIES if e.T) and all(T[e.name] < 1 and e.T == 0 for e in WL.TOO_SHORT)
    # 32-frame LayerNorm blocks, the 64-frame pitch (tp == T exactly at 64 and 256), the 256-key attention block
    for lo, mid, hi, blk in (("T31", "T32", "T33", 32), ("T63", "T64", "T65", 64), ("T255", "T256", "T257", 256)):
        assert (T[lo], T[mid], T[hi]) == (blk - 1, blk, blk + 1)
    for name in ("T64", "T256", "T64+159", "T256+159", "B2_T64"):
        assert (T[name] + 63) // 64 * 64 == T[name]
    # positional conv: piece s reads frames t + 11 s - 64 .. t + 11 s - 54; up to 57 frames the last piece (s = 11: t + 57 ..) is wholly
    # outside, up to 54 the first (.. t - 54), at T = 1 every piece but s = 5 (window -9 .. 1)
    outside = lambda Tn, s: all(not (0 <= t + 11 * s - 64 + j < Tn) for t in range(Tn) for j in range(11))
    assert outside(57, 11) and not outside(58, 11) and outside(54, 0) and not outside(55, 0)
    assert all(outside(T[n], 11) and outside(T[n], 0) for n in ("T1", "T2", "T3", "T31", "T32", "T33")) and not outside(63, 11)
    assert [s for s in range(12) if not outside(1, s)] == [5]
    assert all(64 - 11 * s < 0 for s in range(6, 12)) and 64 - 11 * 5 > 0
    # off-grid
    off = WL.BY_NAME
    assert fe_lens(1044) == fe_lens(1040) and (1044 - 10) % 5 == 4
    assert off["off16123"].n % 5 == 3 and T["off16123"] == 50
    assert [(off[f"T{t}+159"].n, T[f"T{t}+159"]) for t in (2, 32, 64, 256)] == [(879, 2), (10479, 32), (20719, 64), (82159, 256)]
    assert all(e.n % 5 for e in WL.OFF_GRID)
    # too short
    assert fe_lens(399)[-1] == 0 and fe_lens(400)[-1] == 1 and fe_lens(9)[0] == 0
    # batches
    assert [(e.B, T[e.name]) for e in WL.BATCHES] == [(3, 2), (3, 33), (2, 64), (2, 32)]
    assert [(WL.BY_NAME[name].n, WL.BY_NAME[name].B, step) for name, step in WL.CONVERT] == [(16123, 1, 1), (20560, 1, 4), (10320, 2, 1)]
    assert len({e.name for e in WL.ENTRIES}) == len(WL.ENTRIES)
    seeds = [s for e in WL.ENTRIES for s in e.seeds()]
    assert len(set(seeds)) == len(seeds)


def test_fixture_matches_the_catalogue(gold):
    fx = WL.fixture(gold)
    for e in WL.ENTRIES:
        if e.T == 0:
            assert str(fx[f"{e.name}/raises"]) in ("RuntimeError", "ValueError"), e
            assert f"{e.name}/idx" not in fx
            continue
        assert f"{e.name}/raises" not in fx, e
        assert fx[f"{e.name}/bn_shape"].tolist() == [e.B, 256, e.T + 1], e          # 256 dims, the replicate-padded frame
        assert fx[f"{e.name}/idx"].shape == fx[f"{e.name}/margin"].shape == fx[f"{e.name}/d1"].shape == fx[f"{e.name}/znorm"].shape == (e.B, e.T + 1)
        assert fx[f"{e.name}/w2v2_last_sub"].shape == (e.B, e.T, 64)
        assert (fx[f"{e.name}/margin"] >= 0).all() and 0 <= fx[f"{e.name}/idx"].min() and fx[f"{e.name}/idx"].max() < 48
        if e.edge == "parity":
            assert fx[f"{e.name}/fe_sub"].shape == (1, 3, 128)
    for name, step in WL.CONVERT:
        e = WL.BY_NAME[name]
        assert f"{name}/convert_raises" not in fx           # the reference's YAAPT tracks all three lengths
        w = fx[f"{name}/convert"]
        assert w.shape[0] == e.B and w.shape[-1] == len(range(0, (e.T + 1) * 320 + 1, step)), (name, w.shape)


def test_reference_margins_leave_the_flip_cap_reachable(gold):
    """the split-f16 extractor may differ from the reference's VQ index only on a frame whose margin its own feature error dz can
    close: d2 - d1 <= 2 dz (sqrt d1 + sqrt d2) + 2 dz^2, at most FLIP_CAP frames per entry.  The cap can only be met if the
    reference itself has no more than that many frames a TYPICAL error closes: dz = sigma_rel |z| with sigma_rel = 1.07e-5, the
    relative feature error DESIGN.md records for the split-f16 wav2vec2 extractor against its exact twin (`asrbn._tie_guard`).  Printed:
    the frames inside the product's own tie window of 4 sigma, which the delivered indices decide again on the exact kernels"""
    fx = WL.fixture(gold)
    sigma_rel, inside4 = 1.07e-5, {}
    for e in WL.ENTRIES:
        if e.T == 0:
            continue
        d1 = fx[f"{e.name}/d1"].astype(np.float64).clip(min=0)
        m = fx[f"{e.name}/margin"].astype(np.float64)
        zn = fx[f"{e.name}/znorm"].astype(np.float64)
        assert zn.shape == m.shape and (zn > 1).all()
        at_risk = lambda dz: m <= 2 * dz * (np.sqrt(d1) + np.sqrt(d1 + m)) + 2 * dz ** 2
        assert at_risk(sigma_rel * zn).sum() <= WL.FLIP_CAP, (e.name, int(at_risk(sigma_rel * zn).sum()))
        if at_risk(4 * sigma_rel * zn).any():
            inside4[e.name] = (int(at_risk(sigma_rel * zn).sum()), int(at_risk(4 * sigma_rel * zn).sum()))
    print("entries with frames inside (1 sigma, 4 sigma) of the split-f16 feature error:", inside4)


@pytest.mark.parametrize("rounding", ["up_at_layer_2"])
def test_a_wrong_fe_lens_is_told_apart(rounding):
    """the comparison above has teeth: `_fe_lens` rounding up at one stride-2 layer differs from the oracle's counts at every
    length whose frame count into that layer is even (the parity set holds 32 of them)"""
    def wrong(n):
        lens, t = [], n
        for i, (_, k, s) in enumerate(CONV_LAYERS):
            t = -((t - k) // -s) + 1 if i == 2 else (t - k) // s + 1
            lens.append(t)
        return lens
    differ = [e.n for e in WL.PARITY if wrong(e.n) != oracle_layer_frames(e.n)]
    assert len(differ) == 32
