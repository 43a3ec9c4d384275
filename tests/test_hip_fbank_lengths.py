"""The fbank tag end to end over the length catalogue of tests/fbank_lengths.py: what lies BETWEEN the kernels of `TdnnfVqNet` — the frame
count of the features, `pad_input`'s tiled right pad, the form each TDNNF layer is launched in (`asrbn.plan_layers`), the `[:, :, ::2]` of the
stride-2 layer and its strided bypass, the tile shape linearA is dispatched to, the VQ's 64-frame blocks, `pad_replicate` and the
`int(n / 1.5)` bypass of the ASR head, the nearest interpolation of F0 in `convert()` — at every fbank frame count from 3 to 40, on both
sides of every dispatch flip up to 2.6 s, at lengths off the 160-sample grid, in batches of 2, 3 and 5, and below one frame.  Needs a real
MI355X: run with `-m gpu` (`-s` prints every figure; SAT_FBANK_LENGTHS_REPORT names a file for the table of error / bar ratios).

References and bars are the project's own:
  * features: float64 of fbank + CMVN + pad (ref64_w2v2.fbank) within `fbank_bound` of tests/test_hip_w2v2_kernels.py, per element; and the
    reference's recorded bins within the 3e-4 of tests/test_hip_parity.py::test_fbank_cmvn_pad_matches_oracle;
  * a stack layer is taken from the device's OWN input (the `hook` of `_run_layers`, `tdnnf_planes_only` off) and held to float64 of that one
    layer: relative RMS 2e-6 (exact f32) / 5e-6 (split planes), the bars of the sat_tdnnf_layer_f32 row of tests/test_hip_bounds.py; and per
    element LAYER_MARGIN x the largest error of float32 torch on the CPU for the same layer and input (two f32 implementations differ by
    re-association alone), plus on split planes 2^-21 of each product's sum of magnitudes (the split-f16 product drops ~2^-21
    relative), carried through linearA and the BatchNorm scale.  Neither term comes from the kernel's output.  Measured
    (profiles/fbank_length_sweep_run.txt): at most 0.40 of the per-element bar on the eleven full layers; the bottleneck layer in exact f32
    (one 3072-term product, no BatchNorm behind it) comes closest, 0.69 .. 0.95;
  * the whole extractor against the reference's own Net (tests/golden/fx_fbank_lengths*.npz): z < 2e-4, and every VQ index equal where the
    reference's margin exceeds 5e-3 (tests/test_hip_parity.py::_check_extract_bn), at most FLIP_CAP flips per entry below that, none as
    delivered with the near-tie guard at its default;
  * the ASR head at the bars of test_asr_forward_matches_reference (RMS 1e-4, logsumexp 1e-4) and test_asr_forward_of_a_ragged_utterance_list
    (2e-5 of the largest value); convert() at the 1e-4 RMS of test_convert_matches_golden.
Freed device memory is filled with NaN before the runs (`_poison`): a frame nothing writes shows."""
import hashlib
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fbank_lengths as FL
import ref64
import ref64_w2v2 as R
from conftest import rms
from test_hip_w2v2_kernels import _fbank_tables, fbank_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ("f16x3", "f32")
RMS_BAR = {"f32": 2e-6, "f16x3": 5e-6}
LAYER_MARGIN = 8.0          # re-association: the kernel's summation order against torch's, both float32
SPLIT = 2.0 ** -21
Z_BAR, MARGIN_BAR, FB_REF_BAR, WAV_BAR = 2e-4, 5e-3, 3e-4, 1e-4

_RATIO = {}             # (layer, precision) -> (largest error / bar, rel RMS / bar, entry)
_FLIPS = {}             # (entry, precision, planes_only) -> excused flips
_SERVED = {}            # (layer, kernel) -> t_q seen
_ids = lambda e: e.name


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    lines = ["# tests/test_hip_fbank_lengths.py: per stack layer the largest (per-element error / bar, relative RMS / bar) over the layer entries; above 1 fails"]
    lines += [f"{k[0]:10s} {k[1]:6s} element {r:8.5f}  rms {q:8.5f}   at {at}" for k, (r, q, at) in sorted(_RATIO.items())]
    lines.append("# kernels seen serving linearA of each layer on split planes (frame counts)")
    lines += [f"{k[0]:10s} {k[1]:28s} t_q {sorted(v)}" for k, v in sorted(_SERVED.items())]
    for prec in PRECISIONS:
        n = sum(v for k, v in _FLIPS.items() if k[1] == prec)
        lines.append(f"# excused VQ index flips, {prec}: {n} over {sum(1 for k in _FLIPS if k[1] == prec)} runs (cap {FL.FLIP_CAP} per entry)"
                     + "".join(f"  {k[0]}{'/planes-only' if k[2] else ''}: {v}" for k, v in sorted(_FLIPS.items()) if k[1] == prec and v))
    lines.append(f"# module run time {time.time() - t0:.1f} s")
    print("\n" + "\n".join(lines))
    path = os.environ.get("SAT_FBANK_LENGTHS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def model():
    import satools_amd
    m = satools_amd.load_model("synthetic:" + FL.TAG)
    m.to(DEV)
    m.eval()
    return m


@pytest.fixture(scope="module")
def fx(gold):
    return FL.fixture(gold)


@pytest.fixture(scope="module")
def asr_state(fbank_tag_state):
    from oracle import convert as oconv
    return oconv.split_state_dict(fbank_tag_state[0]["base_model_state_dict"])[0]


class _arith:
    """the bottleneck extractor on one arithmetic (and one setting of `tdnnf_planes_only`) for the duration of a block"""

    def __init__(self, ext, prec, planes_only=None):
        self.ext, self.prec, self.planes_only = ext, prec, planes_only

    def __enter__(self):
        self.keep = self.ext.precision
        self.ext.precision = self.prec
        if self.planes_only is not None:
            self.ext.tdnnf_planes_only = self.planes_only

    def __exit__(self, *a):
        self.ext.precision = self.keep
        self.ext.__dict__.pop("tdnnf_planes_only", None)


def _poison():
    """fill what the caching allocator holds free with NaN: `torch.empty` then hands out NaN, not whatever was there"""
    bufs = [torch.full((n,), float("nan"), device=DEV) for n in (1 << 7, 1 << 10, 1 << 13, 1 << 16, 1 << 18, 1 << 20) for _ in range(3)]
    torch.cuda.synchronize()
    del bufs


def _last_kernel():
    from satools_amd import _lib
    return _lib.lib().sat_last_dispatch_name().decode()


# ---- features ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", FL.SMALL + FL.OFF_GRID, ids=_ids)
def test_features_match_float64_and_the_reference_bins(model, fx, entry):
    window, mel, _, _ = _fbank_tables()
    wav = entry.wav()
    _poison()
    got = model.bn_extractor.features(wav.to(DEV).to(torch.float32).contiguous(), scale=32768.0).cpu()
    assert got.shape == (1, 80, entry.F + 2 * FL.PAD) and bool(torch.isfinite(got).all())
    want, a = R.fbank(wav.to(torch.float32), window, mel, scale=32768.0, cmvn=True, pad=FL.PAD)
    err, bound = (got.double() - want).abs(), fbank_bound(a, window, mel, True, FL.PAD)
    r = float((err / bound.clamp(min=1e-300)).max())
    print(f"features {entry.name} n={entry.n} F={entry.F}: max error {float(err.max()):.3e}, max error / bound {r:.4f}")
    if r > _RATIO.get(("features", "f32"), (-1.0,))[0]:
        _RATIO[("features", "f32")] = (r, 0.0, entry.name)
    assert r <= 1.0, (entry.name, r)
    if f"{entry.name}/fbank_sub" in fx:
        ref = torch.from_numpy(fx[f"{entry.name}/fbank_sub"]).double()           # [1, F, 10]: every 8th bin, before the CMVN
        ref = (ref - ref.mean(dim=1, keepdim=True)).permute(0, 2, 1)
        core = got[:, ::8, FL.PAD:FL.PAD + entry.F].double()
        assert float((core - ref).abs().max()) < FB_REF_BAR, entry.name
        # the pads: the first frame, the last frame
        assert torch.equal(got[:, :, :FL.PAD], got[:, :, FL.PAD:FL.PAD + 1].expand(-1, -1, FL.PAD))
        assert torch.equal(got[:, :, FL.PAD + entry.F:], got[:, :, FL.PAD + entry.F - 1:FL.PAD + entry.F].expand(-1, -1, FL.PAD))


# ---- each stack layer against float64 of that layer on the device's own input -----------------------------------------------------------
def _layer(lay, x, dt, bottleneck):
    """one TDNNFBatchNorm (chain/nn.py:267-292, :338-347) on x [B, feat, T] in torch on the CPU at dtype dt -> y (the bottleneck layer: z)
    and, for the split-plane allowance, 2^-21 of each product's sum of magnitudes carried to the output"""
    p = lambda t: t.detach().cpu().to(dt)
    ctx, sub = lay.context_len, int(lay.subsampling_factor)
    wB = p(lay.tdnn.linearB.inner_nat.weight)
    wB = wB.reshape(wB.shape[0], ctx, lay.feat_dim).permute(0, 2, 1).contiguous()
    bB = p(lay.tdnn.linearB.inner_nat.bias).reshape(-1)
    x = x.to(dt)
    z = F.conv1d(x, wB, bB, stride=sub)
    tz = SPLIT * F.conv1d(x.abs(), wB.abs(), bB.abs(), stride=sub)
    if bottleneck:
        return z, tz
    wA, bA = p(lay.tdnn.linearA.weight).unsqueeze(-1), p(lay.tdnn.linearA.bias)
    y = F.conv1d(z, wA, bA)
    ty = F.conv1d(tz, wA.abs()) + SPLIT * F.conv1d(z.abs(), wA.abs(), bA.abs())
    if lay.use_bypass:
        l = ctx // 2 if ctx > 1 else 0
        y = y + ref64.f32(lay.bypass_scale) * x[:, :, l:l + (y.shape[2] - 1) * sub + 1:sub]
    scale = 1.0 / torch.sqrt(p(lay.bn.running_var) + 1e-5)
    shift = -p(lay.bn.running_mean) * scale
    return F.relu(y * scale[None, :, None] + shift[None, :, None]), ty * scale[None, :, None]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("entry", FL.LAYERS + FL.DISPATCH, ids=_ids)
def test_each_stack_layer_against_float64_of_its_own_input(model, entry, prec):
    ext = model.bn_extractor
    lays = ext._stack_layers()
    wav = entry.wav().to(DEV)
    seen = []
    with _arith(ext, prec, planes_only=False):
        _poison()
        feats = ext.features(wav.to(torch.float32).contiguous(), scale=32768.0)
        _, (z, _, _) = ext._run_stack(feats, want_aux=True, hook=lambda name, form, x: seen.append((name, form, x, _last_kernel())))
        torch.cuda.synchronize()
    assert [s[0] for s in seen] == FL.LAYER_NAMES + ["tdnnfs.20"]
    assert [s[1] for s in seen] == (["one_call"] * 3 + [("sub_planes" if prec == "f16x3" else "two_call")] + ["one_call"] * 7 + ["two_call"])
    tq = FL.stack_tq(entry.F)
    x = feats.cpu()
    for i, (lay, (name, form, y, kernel)) in enumerate(zip(lays, seen)):
        last = i + 1 == len(lays)
        got = (z if last else y).cpu().double()
        want, split = _layer(lay, x, torch.float64, last)
        f32, _ = _layer(lay, x, torch.float32, last)
        assert got.shape == want.shape == (1, want.shape[1], tq[i]), (entry.name, name, got.shape, want.shape)
        assert bool(torch.isfinite(got).all()), (entry.name, name)
        bar = LAYER_MARGIN * float((f32.double() - want).abs().max()) + (split if prec == "f16x3" else 0.0)
        err = (got - want).abs()
        r = float((err / bar).max())
        q = rms((got - want).numpy()) / rms(want.numpy()) / RMS_BAR[prec]
        print(f"{entry.name} {prec} {name} ({form}, {kernel.split('<')[0]}, t_q {tq[i]}): max error {float(err.max()):.3e}, / bar {r:.4f}; relative RMS / bar {q:.4f}")
        if r > _RATIO.get((name, prec), (-1.0,))[0]:
            _RATIO[(name, prec)] = (r, max(q, _RATIO.get((name, prec), (0, 0.0))[1]), f"{entry.name} t_q {tq[i]}")
        assert r <= 1.0 and q <= 1.0, (entry.name, prec, name, r, q)
        if form == "one_call":          # the layer's last launch is linearA: which tile shape served it
            want_kernel = "conv1d_mfma_kernel" if prec == "f32" else "gemm_f16x3_ring16_kernel" if FL.cols256(tq[i]) else "conv1d_f16x3_k1_kernel"
            assert kernel.startswith(want_kernel), (entry.name, prec, name, tq[i], kernel)
        x = got.float() if not last else None


def test_both_kernels_are_seen_serving_every_one_call_layer(model):
    """over the dispatch-edge entries on split planes each one-call layer's linearA runs on the 128 x 256 ring GEMM and on the 128 x 128 GEMM,
    next to each flip: the kernel named by the library after the layer's last launch"""
    ext = model.bn_extractor
    with _arith(ext, "f16x3", planes_only=False):
        for e in FL.DISPATCH:
            tq = iter(FL.stack_tq(e.F))
            feats = ext.features(e.wav().to(DEV).contiguous(), scale=32768.0)
            ext._run_stack(feats, hook=lambda name, form, x: _SERVED.setdefault((name, _last_kernel().split("<")[0]), set()).add(next(tq)))
    for i, name in enumerate(FL.LAYER_NAMES):
        if i == 3:
            continue
        ring, k1 = _SERVED.get((name, "gemm_f16x3_ring16_kernel"), set()), _SERVED.get((name, "conv1d_f16x3_k1_kernel"), set())
        assert 129 in ring and {127, 128} <= k1, (name, sorted(ring), sorted(k1))
        if i < 3:
            assert 256 in ring and 257 in k1, (name, sorted(ring), sorted(k1))


# ---- the whole extractor on every entry ---------------------------------------------------------------------------------------------------
def _check_indices(entry, fx, idx, key, guarded=False):
    ref = torch.from_numpy(fx[f"{entry.name}/idx"].astype(np.int64))
    margin = torch.from_numpy(fx[f"{entry.name}/margin"])
    agree = idx.cpu().long() == ref
    flips = int((~agree).sum())
    assert agree[margin > MARGIN_BAR].all(), (entry.name, key, torch.nonzero(~agree).tolist(), margin[~agree].tolist())
    assert flips <= (0 if guarded else FL.FLIP_CAP), (entry.name, key, torch.nonzero(~agree).tolist(), margin[~agree].tolist())
    if flips:
        print(f"{entry.name} {key}: {flips} excused VQ index flips at margins {margin[~agree].tolist()}")
    if not guarded:
        _FLIPS[(entry.name,) + key] = flips
    return agree


@pytest.mark.parametrize("entry", FL.RUNNING, ids=_ids)
def test_whole_extractor_matches_the_reference(model, fx, entry):
    ext = model.bn_extractor
    wav = entry.wav()
    zref = torch.from_numpy(fx[f"{entry.name}/z_sub"])          # [B, T, 16]
    for prec in PRECISIONS:
        idxs = {}
        for planes_only in (True, False):
            with _arith(ext, prec, planes_only):
                _poison()
                bn, (z, idx, _) = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
                torch.cuda.synchronize()
            assert list(bn.permute(0, 2, 1).shape) == fx[f"{entry.name}/bn_shape"].tolist() == [entry.B, 256, entry.T]
            assert z.shape == (entry.B, 256, entry.T) and idx.shape == (entry.B, entry.T) and bool(torch.isfinite(z).all())
            ez = float((z.cpu().permute(0, 2, 1)[..., ::16] - zref).abs().max())
            print(f"{entry.name} {prec} planes_only={planes_only}: z max abs error vs the reference {ez:.3e}")
            assert ez < Z_BAR, (entry.name, prec, planes_only, ez)
            _check_indices(entry, fx, idx, (prec, planes_only))
            idxs[planes_only] = idx.cpu()
        assert torch.equal(idxs[True], idxs[False]), (entry.name, prec)
    # as delivered: the default arithmetic with the near-tie guard at its default
    assert ext.precision == "f16x3" and ext.vq_tie_sigmas == 4.0
    idx, _ = ext.vq_indices(wav.to(DEV))
    _check_indices(entry, fx, idx, ("f16x3", "guarded"), guarded=True)


@pytest.mark.parametrize("entry", FL.BATCHES, ids=_ids)
def test_rows_of_a_batch_are_the_oracles_batch(model, fx, asr_state, entry):
    """get_bn of a batch against the oracle's run of the same batch (pad_input's tiled right pad couples the rows: a single-utterance run
    pads differently and is no reference here), all 256 dimensions"""
    from oracle import tdnnf as otd
    wav = entry.wav()
    aux = {}
    ref = otd.extract_bn_fbank(asr_state, wav, aux=aux).permute(0, 2, 1)          # [B, 256, T]
    assert np.array_equal(aux["idx"].numpy(), fx[f"{entry.name}/idx"])
    for prec in PRECISIONS:
        with _arith(model.bn_extractor, prec):
            _poison()
            w = wav.to(DEV)
            bn = model.get_bn(w).cpu()
            assert torch.equal(w.cpu(), wav)
            idx, _ = model.bn_extractor.vq_indices(wav.to(DEV))
        assert bn.shape == ref.shape == (entry.B, 256, entry.T)
        agree = _check_indices(entry, fx, idx, (prec, "batch"), guarded=True)
        err = float((bn - ref).permute(0, 2, 1)[agree].abs().max())
        print(f"{entry.name} {prec}: get_bn of the batch vs the oracle's batch, max abs error {err:.3e}")
        assert err < Z_BAR, (entry.name, prec, err)


# ---- error behaviour --------------------------------------------------------------------------------------------------------------------
def test_too_short_raises_like_the_reference(model, fx):
    """the reference's scripted fbank fails its assert (torch.jit.Error: "RuntimeError: AssertionError: choose a window size 400 that is
    [2, n]"); every entry point here raises a RuntimeError with that sentence"""
    ext = model.bn_extractor
    for e in FL.TOO_SHORT:
        said = str(fx[f"{e.name}/raises"][1])
        assert said.startswith("RuntimeError: ") and said.endswith(f"choose a window size 400 that is [2, {e.n}]")
        for call in (lambda w: ext.extract_bn(w), lambda w: model.get_bn(w), lambda w: ext.forward(w), lambda w: ext.forward_ragged([w[0]])):
            with pytest.raises(RuntimeError, match=rf"choose a window size 400 that is \[2, {e.n}\]"):
                call(e.wav().to(DEV))
    for name in FL.CONVERT_RAISES:          # the reference's YAAPT fails on a track of two frames
        assert str(fx[f"{name}/convert_raises"][0]) == "RuntimeError"
        e = FL.BY_NAME[name]
        with pytest.raises(RuntimeError):
            model.convert(e.wav().to(DEV), target=FL.convert_targets(model.spk, e.B))
        model.get_bn(e.wav().to(DEV))          # (and the extractor goes on working)


# ---- the ASR head -------------------------------------------------------------------------------------------------------------------------
def _head_close(got, fx, name, row=None):
    chain, xent = got
    for t, key in ((chain, "chain_sub"), (xent, "xent_sub")):
        want = fx[f"{name}/{key}"] if row is None else fx[f"{name}/{key}"][row]
        g = t.cpu().numpy()[..., ::16]
        assert g.shape == want.shape, (name, key, g.shape, want.shape)
        assert rms(g - want) <= 1e-4 * max(1.0, rms(want)), (name, key, rms(g - want))
    lse = fx[f"{name}/xent_lse"] if row is None else fx[f"{name}/xent_lse"][row]
    assert np.allclose(torch.logsumexp(xent, dim=-1).cpu().numpy(), lse, atol=1e-4), name


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("entry", FL.ASR, ids=_ids)
def test_asr_forward_matches_the_reference(model, fx, entry, prec):
    ext = model.bn_extractor
    with _arith(ext, prec):
        _poison()
        chain, xent = ext.forward(entry.wav().to(DEV))
    assert chain.shape == xent.shape == (entry.B, FL.head_frames(entry.T), 3280) and bool(torch.isfinite(chain).all())
    _head_close((chain, xent), fx, entry.name)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("names", FL.RAGGED, ids=lambda r: "+".join(r))
def test_asr_forward_ragged_is_forward_of_each_utterance(model, fx, names, prec):
    ext = model.bn_extractor
    wavs = [FL.BY_NAME[n].wav()[0].to(DEV) for n in names]
    with _arith(ext, prec):
        _poison()
        got = ext.forward_ragged(wavs)
        for i, (n, w) in enumerate(zip(names, wavs)):
            c1, x1 = ext.forward(w.reshape(1, -1).clone())
            assert got[i][0].shape == c1[0].shape == (FL.head_frames(FL.BY_NAME[n].T), 3280) and got[i][1].shape == x1[0].shape, (n, got[i][0].shape)
            ec, ex = (got[i][0] - c1[0]).abs().max().item(), (got[i][1] - x1[0]).abs().max().item()
            print(f"forward_ragged {prec} {n}: chain {ec:.2e} of {c1.abs().max().item():.1f}, xent {ex:.2e} of {x1.abs().max().item():.1f}")
            assert ec < 2e-5 * max(1.0, c1.abs().max().item()) and ex < 2e-5 * max(1.0, x1.abs().max().item()), (n, ec, ex)
    assert FL.BY_NAME[names[0]] in FL.ASR
    _head_close(got[0], fx, names[0], row=0)


# ---- convert() ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FL.CONVERT)
def test_convert_matches_the_reference_waveform(model, fx, name):
    e = FL.BY_NAME[name]
    wav, ref, f0 = e.wav(), fx[f"{name}/convert"], torch.from_numpy(fx[f"{name}/f0"].copy())
    tg = FL.convert_targets(model.spk, e.B)
    got_f0 = model.get_f0(wav.to(DEV)).cpu()
    assert got_f0.shape == f0.shape == (e.B, FL.f0_frames(e.n)) and FL.f0_frames(e.n) - e.T in (0, 1)
    assert torch.equal(got_f0[:, 1:], f0[:, 1:]), name          # (frame 0 depends on the thread count in the reference: tests/test_hip_robust.py)
    for how in ("set_f0", "own"):
        if how == "set_f0":
            model.set_f0(f0.clone().to(DEV))
        _poison()
        y = model.convert(wav.to(DEV), target=tg).cpu().numpy()
        assert y.shape == ref.shape and y.shape[-1] == e.T * 320 + 1, (name, y.shape, ref.shape)
        err = rms(y - ref)
        print(f"convert {name} ({how}): RMS error vs the reference {err:.2e}, signal RMS {rms(ref):.2e}")
        assert err < WAV_BAR, (name, how, err)
    assert model.f0 is None


def test_convert_padded_of_a_ragged_list(model, fbank_tag_state):
    """convert_padded of a zero-padded ragged list: each row's F0 track is that of the row's own samples, and the waveform is the oracle's
    convert() of the same padded batch fed those tracks (the padding and pad_input couple the rows, so a one-utterance convert() is no
    reference for a row: tests/test_hip_robust.py::test_ragged_1_to_35_s_batch_through_process_data)"""
    from oracle import convert as oconv
    names = FL.RAGGED[0]
    es = [FL.BY_NAME[n] for n in names]
    lens = [e.n for e in es]
    x = torch.zeros(len(es), max(lens))
    for i, e in enumerate(es):
        x[i, :e.n] = e.wav()[0]
    tg = [model.spk[3 + 7 * i] for i in range(len(es))]
    tracks = [model.get_f0(x[i:i + 1, :n].contiguous().to(DEV))[0].cpu() for i, n in enumerate(lens)]
    f0 = torch.zeros(len(es), max(t.shape[0] for t in tracks))
    for i, t in enumerate(tracks):
        f0[i, :t.shape[0]] = t
    _poison()
    got = model.convert_padded(x.to(DEV), lens, tg).cpu()
    want = oconv.convert_fbank(fbank_tag_state[0]["base_model_state_dict"], model.spk, x, tg, f0)
    assert got.shape == want.shape
    for i, n in enumerate(lens):
        err = rms(got[i, 0, :n].numpy() - want[i, 0, :n].numpy())
        print(f"convert_padded row {names[i]} (n = {n}): RMS error vs the oracle {err:.2e}")
        assert err < 1e-5, (names[i], err)


# ---- assemble_input ------------------------------------------------------------------------------------------------------------------------
def test_assemble_input_on_every_f0_bottleneck_pair(model):
    """every (T_f0, T) pair the catalogue's lengths produce: the nearest interpolation (f32 scale T_f0 / T) equals F.interpolate's bit for bit"""
    from satools_amd import ops
    pairs = sorted({(FL.f0_frames(e.n), e.T) for e in FL.RUNNING})
    assert {a - b for a, b in pairs} == {0, 1}
    g = torch.Generator().manual_seed(7)
    for T_f0, T in pairs:
        bn, f0, spk = torch.randn(2, 3, T, generator=g), torch.randn(2, 1, T_f0, generator=g), torch.randn(2, 2, generator=g)
        got = ops.assemble_input(bn.to(DEV), f0.to(DEV), spk.to(DEV), 2).cpu()
        assert torch.equal(got, ref64.assemble_input(bn, f0, spk)), (T_f0, T)
    print(f"assemble_input: {len(pairs)} (T_f0, T) pairs")


# ---- the observation hook changes nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_hook_leaves_the_bits_alone_and_they_are_the_parent_commits(model, gold, prec):
    """`_run_stack` / `_asr_outputs` with and without a hook give the same bits, and get_bn, forward and forward_ragged give the bits of the
    commit before the hook existed: tests/golden/fx_fbank_parent_bits.json holds the SHA-256 of their outputs on two catalogue entries and
    one ragged list, dumped on an MI355X from that commit (a change that alters the arithmetic on purpose records its own digests)"""
    want = gold.json("fx_fbank_parent_bits.json")
    dig = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    ext = model.bn_extractor
    with _arith(ext, prec):
        for name in ("F33", "B2_F92"):
            wav = FL.BY_NAME[name].wav().to(DEV)
            assert dig(model.get_bn(wav.clone())) == want[f"{prec}/get_bn/{name}"], (prec, name)
            c, x = ext.forward(wav.clone())
            assert dig(c) + dig(x) == want[f"{prec}/forward/{name}"], (prec, name)
            feats = ext.features(wav.to(torch.float32).contiguous(), scale=32768.0)
            seen = []
            plain, hooked = ext._run_stack(feats), ext._run_stack(feats, hook=lambda n, f, t: seen.append(n))
            assert torch.equal(plain, hooked) and len(seen) == 12
            plain, hooked = ext._asr_outputs(feats), ext._asr_outputs(feats, hook=lambda n, f, t: seen.append(n))
            assert torch.equal(plain[0], hooked[0]) and torch.equal(plain[1], hooked[1]) and len(seen) == 12 + 12 + 4 + 2
        wavs = [FL.BY_NAME[n].wav()[0].to(DEV) for n in FL.RAGGED[0]]
        assert "".join(dig(c) + dig(x) for c, x in ext.forward_ragged(wavs)) == want[f"{prec}/forward_ragged/0"], prec
