"""The wav2vec2 tag end to end over the length catalogue of tests/w2v2_lengths.py: what lies BETWEEN the kernels of
`TdnnfWav2vec2VqNet.w2v2_features` — `t_out=fe_len[i + 1]`, the phase-split shapes, `x_wrap_channels`, the twelve shifted pieces of the
positional conv, `pad_replicate`, `pad_input`, the TDNNF tail, the VQ — at even frame counts into the stride-2 convs (all 64 parity
patterns), at 1 .. 3 frames, around the 32-frame LayerNorm block, the 64-frame pitch (tp == T) and the 256-key attention block, at
lengths whose last samples belong to no frame, in batches of three, and below one frame.  Needs a real MI355X: run with `-m gpu`
(`-s` prints every figure; SAT_W2V2_LENGTHS_REPORT names a file for the table of error / bar ratios).

References and bars are the project's own:
  * a feature-extractor stage is taken from the device's OWN upstream intermediate (the `hook` of w2v2_features, `ops.unsplit` for planes)
    and held to float64 of that one layer: conv 0 to ref64_w2v2.conv0 within k U S, a LayerNorm to ref64_w2v2.layernorm_channels within
    `ln_bound` (+ what split planes leave) of tests/test_hip_w2v2_kernels.py, a stride-2 conv to ref64_conv's running bound (E0 = 3e-5);
  * the reference's own Net on the catalogue is tests/golden/fx_w2v2_lengths*.npz: last layer < 2e-3 (test_w2v2_last_layer_matches_oracle),
    bottleneck < 5e-4 on agreeing frames (test_extract_bn_matches_reference_fixture), waveform RMS < 1e-4, and the feature extractor's
    output < 1e-4, the bar tests/test_oracle_w2v2.py holds a feature subsample to against the same reference (seven layers of at most
    3e-5 each against float64 of their own input, measured two orders below: profiles/w2v2_length_sweep_run.txt);
  * VQ indices: all equal on the exact-f32 kernels; on the split-f16 ones a frame may differ only where the reference's margin is below
    what that frame's measured feature error can move it (tests/test_hip_robust.py::test_convert_long_utterances_wav2vec2_tag), at most
    FLIP_CAP frames per entry.  The feature error of a differing frame is measured against the CPU oracle (tests/test_oracle_w2v2.py pins
    it to the same fixture), which is run only when a frame differs.
Freed device memory is filled with NaN before every extractor run (`_poison`): a slot a kernel is meant to zero — the odd phase's tail —
shows in every later stage if it does not."""
import hashlib
import os

import numpy as np
import pytest
import torch

import ref64_conv as RC
import ref64_w2v2 as R
import w2v2_lengths as WL
from conftest import rms
from ref64 import U
from test_hip_w2v2_kernels import ln_bound, planes_residual, planes_value

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ("f16x3", "f32")
FE_BAR, LAST_BAR, BN_BAR, WAV_BAR, NOVQ_BAR = 1e-4, 2e-3, 5e-4, 1e-4, 5e-4

_RATIO = {}             # (stage, precision) -> (largest error / bar, entry)
_ENTRY = {}             # (entry, precision) -> {quantity: error / bar}
_EXCUSED = {}           # (entry, precision) -> excused VQ index flips
_ids = lambda e: e.name


@pytest.fixture(scope="module", autouse=True)
def report():
    import time
    t0 = time.time()
    yield
    lines = ["# tests/test_hip_w2v2_lengths.py: largest error / bar (a ratio above 1 fails)", "# per stage of the feature extractor, over the 64 parity lengths x 2 utterances"]
    lines += [f"{k[0]:8s} {k[1]:6s} {r:9.5f}   at {at}" for k, (r, at) in sorted(_RATIO.items())]
    lines.append("# per entry: last layer / 2e-3, bottleneck / 5e-4 (up to 65 frames), excused VQ index flips (cap %d)" % WL.FLIP_CAP)
    for (name, prec), d in sorted(_ENTRY.items()):
        lines.append(f"{name:12s} {prec:6s} " + "  ".join(f"{q} {v:.5f}" for q, v in sorted(d.items())) + f"  excused {_EXCUSED.get((name, prec), 0)}")
    lines.append(f"# excused flips over the whole catalogue: {sum(_EXCUSED.values())}; module run time {time.time() - t0:.1f} s")
    print("\n" + "\n".join(lines))
    path = os.environ.get("SAT_W2V2_LENGTHS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def model():
    import satools_amd
    m = satools_amd.load_model("synthetic:" + WL.TAG)
    m.to(DEV)
    m.eval()
    return m


@pytest.fixture(scope="module")
def fx(gold):
    return WL.fixture(gold)


class _arith:
    """the bottleneck extractor on one arithmetic for the duration of a block"""

    def __init__(self, ext, prec):
        self.ext, self.prec = ext, prec

    def __enter__(self):
        self.keep = {k: getattr(self.ext, k) for k in ("precision", "w2v2_precision")}
        self.ext.precision = self.ext.w2v2_precision = self.prec

    def __exit__(self, *a):
        for k, v in self.keep.items():
            setattr(self.ext, k, v)


def _poison():
    """fill what the caching allocator holds free with NaN: `torch.empty` then hands out NaN, not whatever was there"""
    bufs = [torch.full((n,), float("nan"), device=DEV) for n in (1 << 7, 1 << 10, 1 << 13, 1 << 16, 1 << 18, 1 << 20, 1 << 22) for _ in range(3)]
    torch.cuda.synchronize()
    del bufs


def _ops():
    from satools_amd import ops
    return ops


def _ratio(stage, prec, at, got, want, bound):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (stage, at, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), (stage, prec, at, "non-finite output")
    err = (got - want).abs()
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    r = float(torch.where(b > 0, err / b.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf")))).max())
    print(f"{stage} {prec} [{at}]: max error {float(err.max()):.3e}, max error / bound {r:.5f}")
    if r > _RATIO.get((stage, prec), (-1.0, ""))[0]:
        _RATIO[(stage, prec)] = (r, at)
    assert r <= 1.0, (stage, prec, at, r, float(err.max()))


_PARAMS = []


def _fe_params(model):
    """(conv weight, conv bias, LayerNorm gamma, beta) of the seven feature-extractor layers, CPU float32"""
    if not _PARAMS:
        for blk in model.bn_extractor.preprocessor.feature_extractor.conv_layers:
            _PARAMS.append(tuple(t.detach().cpu().float() for t in (blk.conv.weight, blk.conv.bias, blk.layer_norm.weight, blk.layer_norm.bias)))
    return _PARAMS


def _interleave(ps, L):
    """the phase-split [B, 2 C, ceil(L / 2)] back to [B, C, L]"""
    B, C2, _ = ps.shape
    x = torch.zeros(B, C2 // 2, L, dtype=ps.dtype)
    x[:, :, 0::2] = ps[:, :C2 // 2, :(L + 1) // 2]
    x[:, :, 1::2] = ps[:, C2 // 2:, :L // 2]
    return x


# ---- the feature extractor, stage by stage, on all 64 parity patterns ---------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("entry", WL.PARITY, ids=_ids)
def test_feature_extractor_stages_at_every_parity_pattern(model, fx, entry, prec):
    from satools_amd import synthetic
    ops = _ops()
    ext = model.bn_extractor
    lens = ext._fe_lens(entry.n)
    at = f"{entry.name} n={entry.n} L={lens[:6]}"
    wav = synthetic.harm_batch([entry.seed0, entry.seed0 + 1], entry.n)          # a second utterance behind the first
    params = _fe_params(model)
    acts = {}
    with _arith(ext, prec):
        _poison()
        last = ext.w2v2_features(wav.to(DEV), hook=lambda name, x, xs: acts.__setitem__(name, (x, xs)))
        W0 = ext._w2["fe"][0]
        c0 = ops.w2v2_conv0(wav.to(DEV), W0["w"], W0["b"])          # (the split-f16 path fuses conv 0 into its LayerNorm: the same bits,
        torch.cuda.synchronize()                                   #  tests/test_hip_w2v2_kernels.py::test_w2v2_conv0_ln)
    assert list(acts) == ["ln0"] + [f"{s}{i}" for i in range(1, 7) for s in ("conv", "ln")] + ["proj", "pos", "last"]
    assert acts["last"][0] is last and last.shape == (2, 1024, WL.PARITY_T)
    w, b, _, _ = params[0]
    want, a = R.conv0(wav, w.reshape(512, 10), b, 5)
    assert c0.shape == (2, 512, lens[0])
    _ratio("conv0", prec, at, c0, want, 10 * U * a["S"])
    x_prev = c0.cpu()
    for i in range(7):
        split, L = i < 6, lens[i]
        _, _, gamma, beta = params[i]
        want, a = R.layernorm_channels(x_prev, gamma, beta, 1e-5, True, split)
        bound = ln_bound(a, gamma, beta, 512, True, split)
        x, xs = acts[f"ln{i}"]
        assert (xs is not None) == (prec == "f16x3" and split) and (x is None) == (xs is not None)
        got = planes_value(xs) if xs is not None else x.cpu().double()
        assert got.shape == ((2, 1024, (L + 1) // 2) if split else (2, 512, L)), (at, i, got.shape)
        _ratio(f"ln{i}", prec, at, got, want, bound + planes_residual(want) if xs is not None else bound)
        if split and L % 2:          # the odd phase's tail slot: exactly zero (both halves of the planes)
            assert not got[:, 512:, -1].any(), (at, i)
            if xs is not None:
                assert not xs.cpu()[:, 32:, :, :, -1].any(), (at, i)          # planes [B][C / 16][hi | lo][half][t][8]: channels 512 ..
        if split:
            w, b, _, _ = params[i + 1]
            want, e = RC.epilogue(RC.pre_sum(_interleave(got, L), w, stride=2), bias=b)
            y = acts[f"conv{i + 1}"][0]
            assert acts[f"conv{i + 1}"][1] is None and y.shape == (2, 512, lens[i + 1]), (at, i, y.shape)
            _ratio(f"conv{i + 1}", prec, at, y, want, e)
            x_prev = y.cpu()
    fe = acts["ln6"][0].cpu().permute(0, 2, 1)[:1, :, ::4]
    _ratio("fe_out", prec, at, fe, torch.from_numpy(fx[f"{entry.name}/fe_sub"]), FE_BAR)


# ---- the whole extractor on the frame-count edges, the off-grid lengths and the batches ---------------------------------------------
_ORACLE = {}


def _oracle_z(entry):
    """the CPU oracle's VQ input [B (T + 1), 256] float64 for an entry: run only where an index differs"""
    from oracle import convert as oconv
    from oracle import tdnnf as otd
    from oracle import wav2vec2 as ow
    from satools_amd import synthetic
    if "model" not in _ORACLE:
        state, _ = synthetic.checkpoint(WL.TAG)
        asr, _ = oconv.split_state_dict(state["base_model_state_dict"])
        om = ow.Wav2Vec2Restated(24)
        om.load_state_dict({k[len("preprocessor."):]: v for k, v in asr.items() if k.startswith("preprocessor.")})
        om.eval()
        _ORACLE["model"] = (asr, om)
    asr, om = _ORACLE["model"]
    aux = {}
    otd.extract_bn_w2v2(asr, entry.wav(), aux=aux, model=om)
    return aux["z"].reshape(-1, aux["z"].shape[-1]).double(), aux["idx"].reshape(entry.B, -1)


def _check_indices(entry, prec, fx, z, idx):
    """every VQ index the reference's on the exact kernels; on the split-f16 ones only near-ties inside the frame's own feature error
    may differ, at most FLIP_CAP of them.  -> the flipped (utterance, frame) pairs"""
    ref = torch.from_numpy(fx[f"{entry.name}/idx"].astype(np.int64))
    agree = idx.cpu().long() == ref
    flips = torch.nonzero(~agree.flatten()).flatten()
    if prec == "f32":
        assert agree.all(), f"{entry.name}: the exact-f32 kernels must reproduce every VQ index of the reference; frames {flips.tolist()} differ"
    elif flips.numel():
        z_ref, idx_or = _oracle_z(entry)
        assert torch.equal(idx_or.long(), ref)
        d1 = torch.from_numpy(fx[f"{entry.name}/d1"]).double().flatten().clamp_min(0)
        margin = torch.from_numpy(fx[f"{entry.name}/margin"]).double().flatten()
        dz = (z.permute(0, 2, 1).reshape(-1, z.shape[1]).cpu().double() - z_ref).norm(dim=1)
        bound = 2 * dz * (d1.sqrt() + (d1 + margin).sqrt()) + 2 * dz ** 2
        print(f"{entry.name} {prec}: VQ index flips {flips.tolist()}; the reference's margins {[f'{g:.1e}' for g in margin[flips].tolist()]} vs what the "
              f"frame's feature error allows {[f'{g:.1e}' for g in bound[flips].tolist()]}; feature error median {float(dz.median()):.1e}, max {float(dz.max()):.1e}")
        assert (margin[flips] <= bound[flips]).all(), f"{entry.name}: an index differs where the reference's decision was no tie within the kernel's own error"
        assert flips.numel() <= WL.FLIP_CAP, (entry.name, flips.tolist())
    _EXCUSED[(entry.name, prec)] = int(flips.numel())
    return agree


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("entry", WL.WHOLE + WL.BATCHES, ids=_ids)
def test_whole_extractor_matches_the_reference(model, fx, entry, prec):
    ext = model.bn_extractor
    wav = entry.wav()
    with _arith(ext, prec):
        _poison()
        last = ext.w2v2_features(wav.to(DEV)).cpu()
        bn, (z, idx, _) = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
        torch.cuda.synchronize()
    want = torch.from_numpy(fx[f"{entry.name}/w2v2_last_sub"])          # [B, T, 64]: every 16th channel
    assert last.shape == (entry.B, 1024, entry.T) and bool(torch.isfinite(last).all())
    err = float((last.permute(0, 2, 1)[:, :, ::16] - want).abs().max())
    print(f"{entry.name} {prec}: last layer max abs error {err:.3e} (values up to {float(want.abs().max()):.1f})")
    rec = _ENTRY.setdefault((entry.name, prec), {})
    rec["last"] = err / LAST_BAR
    assert err < LAST_BAR
    assert list(bn.permute(0, 2, 1).shape) == fx[f"{entry.name}/bn_shape"].tolist() == [entry.B, 256, entry.T + 1]
    agree = _check_indices(entry, prec, fx, z, idx)
    if f"{entry.name}/bn_sub" in fx:
        d = (bn.cpu().permute(0, 2, 1)[:, ::16] - torch.from_numpy(fx[f"{entry.name}/bn_sub"])).abs()          # [B, 16, T + 1]
        e_bn = float(d.permute(0, 2, 1)[agree].max())
        print(f"{entry.name} {prec}: bottleneck max abs error {e_bn:.3e}")
        rec["bn"] = e_bn / BN_BAR
        assert e_bn < BN_BAR


# ---- batches, off-grid samples, too short ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("entry", WL.BATCHES, ids=_ids)
def test_a_batch_is_its_single_utterances_bit_for_bit(model, entry, prec):
    ext = model.bn_extractor
    wav = entry.wav().to(DEV)
    with _arith(ext, prec):
        _poison()
        full = ext.w2v2_features(wav).clone()
        for j in range(entry.B):
            _poison()
            assert torch.equal(ext.w2v2_features(wav[j:j + 1].contiguous()), full[j:j + 1]), (entry.name, j)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_samples_in_no_frame_change_nothing(model, prec):
    """n = 1044 gives the bits of its first 1040 samples; so does every off-grid length cut back to its grid"""
    ext = model.bn_extractor
    with _arith(ext, prec):
        for e in WL.OFF_GRID:
            wav = e.wav().to(DEV)
            on_grid = 400 + 320 * (e.T - 1)
            assert on_grid < e.n and ext._fe_lens(on_grid)[-1] == e.T
            _poison()
            a = ext.w2v2_features(wav).clone()
            _poison()
            b = ext.w2v2_features(wav[:, :on_grid].contiguous())
            assert torch.equal(a, b), e.name
    assert WL.BY_NAME["off1044"].n == 1044


def test_too_short_raises_and_launches_nothing(model, fx):
    """where the reference raises the extractor refuses, before any kernel of the library is launched: the last dispatch is still the
    marker launch made just before"""
    from satools_amd import _lib
    ops = _ops()
    ext = model.bn_extractor
    for e in WL.TOO_SHORT:
        assert str(fx[f"{e.name}/raises"]) == "RuntimeError"
        wav = e.wav().to(DEV)
        for call in (ext.extract_bn, ext.features, model.get_bn):
            ops.tanh_(torch.zeros(8, device=DEV))
            assert _lib.lib().sat_last_dispatch_name().decode().startswith("tanh_kernel")
            with pytest.raises(_lib.SatError, match="too short"):
                call(wav.clone())
            assert _lib.lib().sat_last_dispatch_name().decode().startswith("tanh_kernel"), e.name


# ---- convert() ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,step", WL.CONVERT, ids=lambda v: str(v))
def test_convert_matches_the_reference_waveform(model, fx, name, step):
    e = WL.BY_NAME[name]
    wav = e.wav().to(DEV)
    _poison()
    y = model.convert(wav, target=WL.convert_targets(model.spk, e.B)).cpu()
    ref = fx[f"{name}/convert"]
    assert y.shape[-1] == (e.T + 1) * 320 + 1 and y.numpy()[..., ::step].shape == ref.shape
    idx, _ = model.bn_extractor.vq_indices(wav)
    flips = torch.nonzero(idx.cpu().long() != torch.from_numpy(fx[f"{name}/idx"].astype(np.int64)))
    assert flips.shape[0] <= WL.FLIP_CAP
    keep = torch.ones(e.B, y.shape[-1], dtype=torch.bool)          # away from flipped frames: a flipped code changes ~40 frames around it
    for bi, t in flips.tolist():
        keep[bi, max(0, (t - 40) * 320):(t + 40) * 320] = False
    diff = (y.numpy()[..., ::step] - ref).reshape(e.B, -1)[keep[:, ::step].numpy()]
    err = rms(diff)
    print(f"convert {name}: RMS error vs the reference {err:.2e} on {diff.size} samples, {flips.shape[0]} flipped frames")
    _ENTRY.setdefault((name, "f16x3"), {})["convert"] = err / WAV_BAR
    assert err < WAV_BAR


# ---- the tag without a quantiser ---------------------------------------------------------------------------------------------------
def test_tag_without_a_quantiser_on_an_even_pattern_and_at_the_pitch():
    """hifigan_bn_tdnnf_wav2vec2_100h_aug_v1 (extract_bn = linearB's output, no VQ) at 20560 samples (64 frames, tp == T) and at a parity
    length whose six frame counts into the stride-2 convs are all even: the oracle's TDNNF tail on the DEVICE's own padded features"""
    import satools_amd
    from oracle import convert as oconv
    from oracle import tdnnf as otd
    from satools_amd import synthetic
    from satools_amd.wav2vec2 import TdnnfWav2vec2VqNet
    m = satools_amd.load_model("synthetic:" + WL.NOVQ_TAG)
    m.to(DEV)
    m.eval()
    ext = m.bn_extractor
    state, _ = synthetic.checkpoint(WL.NOVQ_TAG)
    asr, _ = oconv.split_state_dict(state["base_model_state_dict"])
    even = [e for e in WL.PARITY if WL.parity_pattern(TdnnfWav2vec2VqNet._fe_lens(e.n)) == (0,) * 6]
    assert len(even) == 1
    for e in (WL.BY_NAME["T64"], even[0]):
        wav = synthetic.harm_batch([e.seed0, e.seed0 + 1], e.n).to(DEV)
        _poison()
        feats = ext.features(wav).cpu()          # [2, 1024, T + 1 + 2 * 3]
        bn = ext.extract_bn(wav.clone()).cpu()
        assert feats.shape == (2, 1024, e.T + 7) and bn.shape == (2, e.T + 1, 256)
        want = otd.run_stack(asr, feats.permute(0, 2, 1), otd.W2V2_KS, otd.W2V2_SUB)
        err = float((bn - want).abs().max())
        print(f"{WL.NOVQ_TAG} n={e.n}: extract_bn max abs error vs the oracle's tail on the device's features {err:.2e}")
        _ENTRY.setdefault((e.name + " novq", "f16x3"), {})["bn"] = err / NOVQ_BAR
        assert err < NOVQ_BAR


# ---- the observation hook changes nothing --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_hook_leaves_the_bits_alone_and_they_are_the_parent_commits(model, gold, prec):
    """w2v2_features with and without a hook gives the same bits, and they are the bits of the commit before the hook existed:
    tests/golden/fx_w2v2_parent_bits.json holds the SHA-256 of the output at 16000 and 80000 samples (2 utterances, both arithmetics) dumped
    on an MI355X from that commit's w2v2_features (a change that alters the extractor's arithmetic on purpose records its own digests)"""
    from satools_amd import synthetic
    want = gold.json("fx_w2v2_parent_bits.json")
    ext = model.bn_extractor
    with _arith(ext, prec):
        for n in (16000, 80000):
            wav = synthetic.harm_batch([0, 1], n).to(DEV)
            plain = ext.w2v2_features(wav).clone()
            seen = []
            hooked = ext.w2v2_features(wav, hook=lambda name, x, xs: seen.append(name))
            assert torch.equal(plain, hooked) and len(seen) == 16
            assert hashlib.sha256(plain.cpu().contiguous().numpy().tobytes()).hexdigest() == want[f"{prec}/{n}"], (prec, n)
