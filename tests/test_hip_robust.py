"""Robustness of the HIP path on corpus-shaped input: the wide YAAPT sweep (integer decisions), long utterances
(LibriSpeech / VoicePrivacy utterances reach ~35 s; the reference pads a batch to its longest, bin/pipeline.py:43-66),
ragged batches through the batch job, sizes off every grid, and the sharded RCCL job in a child process.
Needs a real MI355X: run with `-m gpu`."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = {"frame_length": 35.0, "frame_space": 20.0, "nccf_thresh1": 0.25, "tda_frame_length": 25.0}
FBANK_TAG = "hifigan_bn_tdnnf_600h_vq_48_v1"
W2V2_TAG = "hifigan_bn_tdnnf_wav2vec2_vq_48_v1"


def _oracle_f0(wav):
    from oracle import yaapt as oy
    nt = torch.get_num_threads()
    torch.set_num_threads(1)          # the reference's own YAAPT setting (yaapt.py:27; frame 0 depends on the thread count)
    try:
        return oy.yaapt(wav, OPTS)
    finally:
        torch.set_num_threads(nt)


def _special_utterances(n=48000):
    """inputs that stress YAAPT's decisions: chirps, a DC offset, hard clipping, half silence, a very quiet voice"""
    from satools_amd import synthetic
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    out = {}
    f = 80.0 + 120.0 * t / t[-1]                                    # 80 -> 200 Hz chirp, 5 harmonics
    ph = 2 * np.pi * torch.cumsum(f, 0) / 16000.0
    out["chirp_up"] = sum(0.25 / k * torch.sin(k * ph) for k in range(1, 6))
    f = 300.0 - 180.0 * t / t[-1]
    ph = 2 * np.pi * torch.cumsum(f, 0) / 16000.0
    out["chirp_down"] = sum(0.25 / k * torch.sin(k * ph) for k in range(1, 6))
    h = synthetic.harm_batch([3], n)[0].double()
    out["dc_offset"] = (h + 0.2).clamp(-1, 1)
    out["clipped"] = (h * 6.0).clamp(-1, 1)
    hs = h.clone()
    hs[n // 2:] = 0.0
    out["half_silent"] = hs
    out["quiet"] = h * 0.01
    g = torch.Generator().manual_seed(77)
    out["voice_in_noise"] = (h + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)).clamp(-1, 1)
    return {k: v.to(torch.float32).unsqueeze(0) for k, v in out.items()}


def test_yaapt_wide_sweep_is_frame_exact_against_the_oracle():
    """The 100 extra utterances of tests/golden/make_biquad_order_study.py (`harm` and `rand` seeds 100-149, 5 s: 7 of
    them change F0 frames on a 1-ulp difference of the band-pass prefilter) plus chirps, DC offset, clipping, half
    silence, a quiet voice: every frame but frame 0 bit-identical to the CPU oracle (frame 0's squared-signal NCCF is
    flat at ~1.0 and decided by rounding noise in the reference itself, tests/test_oracle_yaapt.py)."""
    from satools_amd import f0 as f0_hip
    from satools_amd import synthetic
    cases = [(f"harm{s}", synthetic.harm_batch([s], 80000)) for s in range(100, 150)]
    cases += [(f"rand{s}", synthetic.rand_batch(s, 1, 80000)) for s in range(100, 150)]
    cases += list(_special_utterances().items())
    bad, frames, same0 = [], 0, 0
    # the GPU tracks in batches of equal length (utterances are independent: test_f0_batch_equals_single_and_oracle)
    got = {}
    for n in (80000, 48000):
        group = [(k, w) for k, w in cases if w.shape[1] == n]
        for i in range(0, len(group), 25):
            part = group[i:i + 25]
            tr = f0_hip.yaapt(torch.cat([w for _, w in part]).to(DEV), OPTS).cpu().numpy()
            for (k, _), row in zip(part, tr):
                got[k] = row
    for name, wav in cases:
        ref = _oracle_f0(wav).numpy()[0]
        g = got[name]
        assert g.shape == ref.shape, name
        frames += ref.size
        same0 += int(g[0] == ref[0])
        if not np.array_equal(g[1:], ref[1:]):
            bad.append((name, np.flatnonzero(g != ref)[:8].tolist()))
    print(f"YAAPT wide sweep: {len(cases)} utterances, {frames} frames; frame 0 equal on {same0}/{len(cases)}")
    assert not bad, bad
    # frame 0 (exempted above: the reference itself changes it with the torch thread count) in fact agrees with the one-thread oracle on
    # 107 / 107 of these inputs (profiles/r05_vq_flip_rate_and_yaapt_frame0.log); a floor, so that a regression there is seen
    assert same0 >= len(cases) - 4, same0


@pytest.fixture(scope="module")
def fbank_model():
    import satools_amd
    m = satools_amd.load_model("synthetic:" + FBANK_TAG)
    m.to(DEV)
    m.eval()
    return m


def _long_batch(seeds, n):
    """`harm` utterances longer than the generator's 5 s period: seeds change every 5 s segment"""
    from satools_amd import synthetic
    rows = []
    for s in seeds:
        segs = [synthetic.harm_batch([s + 7 * j], 80000)[0] for j in range((n + 79999) // 80000)]
        rows.append(torch.cat(segs)[:n])
    return torch.stack(rows)


@pytest.mark.parametrize("seconds", [20, 35])
def test_convert_long_utterances_fbank_tag(fbank_model, fbank_tag_state, seconds):
    """convert() of 2 x 20 s and 2 x 35 s (the longest LibriSpeech / VoicePrivacy utterances), YAAPT on path, against the
    CPU oracle: F0 frame-exact, waveform RMS error < 1e-5 (bar 1e-4)"""
    from oracle import convert as oconv
    from satools_amd import synthetic
    n = seconds * 16000
    wav = _long_batch([1, 2], n)
    tg = synthetic.targets(fbank_model.spk, [0, 1])
    f0 = _oracle_f0(wav)
    got_f0 = fbank_model.get_f0(wav.to(DEV)).cpu()
    assert torch.equal(got_f0[:, 1:], f0[:, 1:])
    state, _ = fbank_tag_state
    ref = oconv.convert_fbank(state["base_model_state_dict"], fbank_model.spk, wav, tg, f0)
    y = fbank_model.convert(wav.to(DEV), target=tg)
    assert y.shape == ref.shape == (2, 1, n + 1)
    err = rms(y.cpu().numpy() - ref.numpy())
    print(f"fbank tag, 2 x {seconds} s: RMS error vs oracle {err:.2e}")
    assert err < 1e-5


@pytest.mark.parametrize("seconds", [20, 35])
def test_convert_long_utterances_wav2vec2_tag(seconds):
    """the same for the wav2vec2 tag (the reference's default, hubconf.py:69): 999 / 1749 frames through the transformer
    (attention over more than one 256-key block), VQ indices equal to the oracle's, waveform < 1e-4 RMS"""
    import satools_amd
    from oracle import convert as oconv
    from oracle import wav2vec2 as ow
    from satools_amd import synthetic
    n = seconds * 16000
    model = satools_amd.load_model("synthetic:" + W2V2_TAG)
    model.to(DEV)
    model.eval()
    state, _ = synthetic.checkpoint(W2V2_TAG)
    sd = state["base_model_state_dict"]
    wav = _long_batch([3, 4], n)
    tg = synthetic.targets(model.spk, [2, 3])
    f0 = _oracle_f0(wav)
    om = ow.Wav2Vec2Restated(24)
    pfx = "bn_extractor.preprocessor."
    om.load_state_dict({k[len(pfx):]: v for k, v in sd.items() if k.startswith(pfx)})
    om.eval()
    aux = {}
    asr, gen = oconv.split_state_dict(sd)
    from oracle import tdnnf as otd
    bn_ref = otd.extract_bn_w2v2(asr, wav, aux=aux, model=om).permute(0, 2, 1)
    ref = oconv.forward(gen, f0.clone().unsqueeze(0), bn_ref, oconv.spk_one_hot(model.spk, tg))
    # The VQ decision (chain/nn.py:424-459) is an argmin over 48 squared distances per frame.  Index work is exact work: the
    # exact-f32 kernels must reproduce EVERY index of the oracle, and the split-f16 kernels (22-bit products) may differ only
    # on a frame whose two best distances the oracle itself separates by less than what THAT frame's measured feature error
    # can move them: |d_k(z + dz) - d_k(z)| <= 2 |dz| sqrt(d_k) + |dz|^2 for both candidates
    ext = model.bn_extractor
    d2s = torch.sort(aux["dist"].reshape(-1, aux["dist"].shape[-1]).double(), dim=1)[0]
    d_best, d_next = d2s[:, 0].clamp_min(0), d2s[:, 1].clamp_min(0)
    z_ref = aux["z"].reshape(-1, aux["z"].shape[-1]).double()
    flips_by_mode = {}
    for mode in ("f32", "f16x3"):
        keep_cfg = {k: getattr(ext, k) for k in ("precision", "w2v2_precision")}
        try:
            if mode == "f32":
                ext.precision = ext.w2v2_precision = "f32"
            _, (z, idx, _) = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
        finally:
            for k, v in keep_cfg.items():
                setattr(ext, k, v)
        assert keep_cfg["w2v2_precision"] == "f16x3" or mode == "f32"
        agree = idx.cpu().long().flatten() == aux["idx"].long().flatten()
        flips = torch.nonzero(~agree).flatten()
        dz = (z.permute(0, 2, 1).reshape(-1, z.shape[1]).cpu().double() - z_ref).norm(dim=1)
        bound = 2 * dz * (d_best.sqrt() + d_next.sqrt()) + 2 * dz ** 2
        print(f"wav2vec2 tag, 2 x {seconds} s, {mode}: {agree.numel()} frames, {flips.numel()} VQ index flips {flips.tolist()}; their oracle gaps "
              f"{[f'{g:.1e}' for g in (d_next - d_best)[flips].tolist()]} vs what the frame's feature error allows {[f'{g:.1e}' for g in bound[flips].tolist()]}; "
              f"feature error: median {float(dz.median()):.1e}, max {float(dz.max()):.1e} (feature norm {float(z_ref.norm(dim=1).median()):.1f})")
        assert ((d_next - d_best)[flips] <= bound[flips]).all(), "an index differs where the oracle's decision was not a tie within the kernel's own error"
        flips_by_mode[mode] = flips
    assert flips_by_mode["f32"].numel() == 0, "the exact-f32 kernels must reproduce every VQ index of the oracle"
    assert flips_by_mode["f16x3"].numel() <= 2
    flips, agree = flips_by_mode["f16x3"], None
    model.set_f0(f0.clone().to(DEV))
    y = model.convert(wav.to(DEV), target=tg)
    assert y.shape == ref.shape
    # compare away from flipped frames (a flipped code changes ~40 frames of output around it: the generator's receptive field)
    keep = torch.ones(y.shape[0], y.shape[-1], dtype=torch.bool)
    T = aux["idx"].numel() // y.shape[0]
    for f in flips.tolist():
        b, t = divmod(f, T)
        keep[b, max(0, (t - 40) * 320):(t + 40) * 320] = False
    diff = (y.cpu() - ref)[:, 0][keep].numpy()
    err = rms(diff)
    print(f"wav2vec2 tag, 2 x {seconds} s: RMS error vs oracle {err:.2e} on {int(keep.sum())} of {keep.numel()} samples")
    assert err < 1e-4


@pytest.mark.parametrize("tag", [FBANK_TAG, W2V2_TAG])
def test_vq_flip_rate_of_the_default_arithmetic(tag):
    """Index work is exact work (chain/nn.py:424-459): the VQ indices the DEFAULT (split-f16) bottleneck extractor DELIVERS equal those
    of its exact-f32 twin (which reproduces every index of the oracle and of the reference fixtures) on 512 utterances of 5 s, 16 of
    20 s and 8 of 35 s per tag (`harm` voices, seeds disjoint from every fixture) — **0 flips**.  How: the VQ kernel counts, per
    utterance, the frames whose two best codes lie inside `vq_tie_sigmas` standard deviations of the arithmetic's calibrated feature
    error (sat_vq_argmin_gather_tie_f32), and those utterances are decided again on the exact kernels (asrbn.resolve_ties).  PRINTED
    (profiles/r06_vq_flips_and_reruns.log keeps the round's figures): the share of utterances decided again, and what the raw
    arithmetic would have flipped without the guard (rounds 1-5: 19 / 13 per million frames)."""
    import satools_amd
    from satools_amd import synthetic
    model = satools_amd.load_model("synthetic:" + tag)
    model.to(DEV)
    model.eval()
    ext = model.bn_extractor
    tot = {"frames": 0, "flips": 0, "raw_flips": 0, "utterances": 0, "rerun": 0, "changed": 0}
    sets = [("5 s", [synthetic.harm_batch(list(range(3000 + 32 * i, 3032 + 32 * i)), 80000) for i in range(16)]),
            ("20 s", [_long_batch(list(range(4000 + 4 * i, 4004 + 4 * i)), 20 * 16000) for i in range(4)]),
            ("35 s", [_long_batch(list(range(5000 + 2 * i, 5002 + 2 * i)), 35 * 16000) for i in range(4)])]
    for name, batches in sets:
        sub = {k: 0 for k in tot}
        for wav in batches:
            wd = wav.to(DEV)
            ext.__dict__.pop("tie_stats", None)
            idx, rows = ext.vq_indices(wd)
            _, (_, idx_raw, _) = ext.extract_bn(wd.clone(), want_aux=True)
            with ext._exact(ext):
                _, (_, idx32, _) = ext.extract_bn(wd.clone(), want_aux=True)
            sub["frames"] += idx.numel()
            sub["flips"] += int((idx != idx32).sum())
            sub["raw_flips"] += int((idx_raw != idx32).sum())
            sub["utterances"] += wd.shape[0]
            sub["rerun"] += ext.tie_stats["rerun"]
            sub["changed"] += len(rows)
        print(f"VQ indices, {tag}, {sub['utterances']} x {name}: {sub['flips']} flips in {sub['frames']} frames; "
              f"{sub['rerun']} utterances decided again on the exact kernels ({100.0 * sub['rerun'] / sub['utterances']:.1f} %), {sub['changed']} of them changed; "
              f"the raw arithmetic: {sub['raw_flips']} flips = {1e6 * sub['raw_flips'] / sub['frames']:.0f} per million")
        for k in tot:
            tot[k] += sub[k]
    print(f"VQ indices, {tag}, all: {tot['flips']} flips in {tot['frames']} frames; {tot['rerun']} of {tot['utterances']} utterances decided again "
          f"({100.0 * tot['rerun'] / tot['utterances']:.1f} %), {tot['changed']} changed; the raw arithmetic: {tot['raw_flips']} flips = {1e6 * tot['raw_flips'] / tot['frames']:.0f} per million "
          f"(window {ext.vq_tie_sigmas} sigma, sigma_rel {ext._tie[2]:.2e})")
    assert tot["flips"] == 0, tot
    assert tot["rerun"] <= 0.08 * tot["utterances"], tot          # (5 s utterances: a few per cent; 35 s utterances carry 7 x the frames each)


def test_convert_20s_wav2vec2_tag_against_the_reference_fixture(gold):
    """the long path of the wav2vec2 tag pinned to the REFERENCE itself (tests/golden/fx_w2v2_long.npz: the reference's own Net on
    one 20 s utterance, 999 frames, made by make_fixtures.py --only w2v2_long): VQ indices, last-layer features, F0 track and
    the waveform of convert().  The exact-f32 kernels reproduce every index; the split-f16 kernels may differ only where the
    reference's two best distances are closer than the kernel's own measured error (its distance to its exact-f32 twin)"""
    import satools_amd
    from satools_amd import synthetic
    fx = gold.npz("fx_w2v2_long.npz")
    n = int(fx["n"])
    wav = torch.cat([synthetic.harm_batch([int(sd)], 80000)[0] for sd in fx["seeds"]])[:n].unsqueeze(0)
    model = satools_amd.load_model("synthetic:" + W2V2_TAG)
    model.to(DEV)
    model.eval()
    ext = model.bn_extractor
    ref_idx = torch.from_numpy(fx["idx"]).long().flatten()
    d1, d2 = torch.from_numpy(fx["d1"]).double().flatten().clamp_min(0), torch.from_numpy(fx["d2"]).double().flatten().clamp_min(0)
    zs, flips = {}, {}
    for mode in ("f32", "f16x3"):
        keep_cfg = {k: getattr(ext, k) for k in ("precision", "w2v2_precision")}
        try:
            if mode == "f32":
                ext.precision = ext.w2v2_precision = "f32"
            _, (z, idx, _) = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
        finally:
            for k, v in keep_cfg.items():
                setattr(ext, k, v)
        zs[mode] = z.permute(0, 2, 1).reshape(-1, z.shape[1]).cpu().double()
        flips[mode] = torch.nonzero(idx.cpu().long().flatten() != ref_idx).flatten()
    dz = (zs["f16x3"] - zs["f32"]).norm(dim=1)
    bound = 2 * dz * (d1.sqrt() + d2.sqrt()) + 2 * dz ** 2
    print(f"20 s wav2vec2 fixture: {ref_idx.numel()} frames; index flips vs the reference: exact-f32 kernels {flips['f32'].tolist()}, split-f16 kernels "
          f"{flips['f16x3'].tolist()} (reference gaps {[f'{g:.1e}' for g in (d2 - d1)[flips['f16x3']].tolist()]}, allowed by the measured error "
          f"{[f'{g:.1e}' for g in bound[flips['f16x3']].tolist()]}); |z_f16x3 - z_f32| median {float(dz.median()):.1e} max {float(dz.max()):.1e}")
    assert flips["f32"].numel() == 0
    assert flips["f16x3"].numel() <= 2 and ((d2 - d1)[flips["f16x3"]] <= bound[flips["f16x3"]]).all()
    feats = ext.w2v2_features(wav.to(DEV))                      # [1, 1024, 999]
    got = feats.permute(0, 2, 1)[:, :, ::16].cpu().double()
    ref = torch.from_numpy(fx["w2v2_last_sub"]).double()
    rel = float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"20 s wav2vec2 fixture: last-layer features relative RMS {rel:.2e}")
    assert rel < 2e-5
    f0 = model.get_f0(wav.to(DEV)).cpu()
    assert np.array_equal(f0.numpy()[:, 1:], fx["f0"][:, 1:])
    y = model.convert(wav.to(DEV), target=model.spk[5])
    assert y.shape == (1, n + 1)                                  # (B = 1: [1, n'], hifigan.py:99-102)
    ref_y = torch.from_numpy(fx["convert_every4"]).reshape(1, 1, -1)
    got_y = y.cpu().reshape(1, 1, -1)[..., ::4]
    assert got_y.shape == ref_y.shape
    keep = torch.ones(got_y.shape[-1], dtype=torch.bool)
    for f in flips["f16x3"].tolist():                           # (a flipped code changes ~40 frames of output around it)
        keep[max(0, (f - 40) * 80):(f + 40) * 80] = False
    err = rms((got_y - ref_y)[0, 0][keep].numpy())
    print(f"20 s wav2vec2 fixture: waveform RMS error vs the reference {err:.2e} on {int(keep.sum())} of {keep.numel()} stored samples")
    assert err < 1e-4


def test_ragged_1_to_35_s_batch_through_process_data(tmp_path, fbank_model):
    """a batch of 1 s ... 35 s utterances through the batch job (zero-pad collate to the longest, per-utterance F0, crop,
    PCM16): every file equals convert_padded() of the same batch, and utterance by utterance the one-utterance convert()
    of the CPU oracle fed with the same per-utterance F0 track (< 1 PCM step RMS)"""
    from oracle import convert as oconv
    from pipeline_toy import read_wav, write_wav
    from satools_amd import pipeline as pl
    from satools_amd import synthetic
    data = str(tmp_path / "data" / "ragged")
    os.makedirs(os.path.join(data, "clear"), exist_ok=True)
    lens = [16000, 35 * 16000, 7 * 16000 + 123, 20 * 16000 + 1]
    scp, u2s, wavs = [], [], []
    for i, n in enumerate(lens):
        x = _long_batch([10 + i], n)[0]
        wavs.append(x)
        path = os.path.join(data, "clear", f"utt{i}.wav")
        write_wav(path, x.numpy().astype(np.float64))
        scp.append(f"utt{i} {path}\n")
        u2s.append(f"utt{i} src{i % 2}\n")
    open(os.path.join(data, "wav.scp"), "w").writelines(scp)
    open(os.path.join(data, "utt2spk"), "w").writelines(u2s)
    target = fbank_model.spk[11]
    settings = types.SimpleNamespace(model="-", f0_modification="", target_constant_spkid=target, results_dir="wav",
                                     batch_size=4, data_loader_nj=2, new_datadir_suffix="_anon", device="cuda")
    table = pl.read_wav_scp(os.path.join(data, "wav.scp"))
    assert pl.process_data(data, "constant", table, settings, model=fbank_model) == 4
    # what the files hold: the PCM16 round trip of the wav files read back (the job's own input)
    x = torch.zeros(4, max(lens))
    for i, n in enumerate(lens):
        x[i, :n] = pl.load_wav_from_scp(table[f"utt{i}"])[0][0]
    ref = fbank_model.convert_padded(x.to(DEV), lens, [target] * 4).cpu()
    for i, n in enumerate(lens):
        got, sr = read_wav(os.path.join(data + "_anon", "wav", f"utt{i}.wav"))
        exp = np.clip(np.rint(ref[i, 0, :n].numpy().astype(np.float64) * 32768), -32768, 32767).astype(np.int16)
        assert sr == 16000 and got.shape == (n,) and np.array_equal(got, exp), i
    # against the oracle: the batch couples its utterances only through the F0 normalisation (cmvn.py:147-151) and the
    # padding; the oracle runs the same padded batch with the per-utterance tracks
    tracks = [_oracle_f0(x[i:i + 1, :n].contiguous())[0] for i, n in enumerate(lens)]
    f0 = torch.zeros(4, max(t.shape[0] for t in tracks))
    for i, t in enumerate(tracks):
        f0[i, :t.shape[0]] = t
    state, _ = synthetic.checkpoint(FBANK_TAG)
    oref = oconv.convert_fbank(state["base_model_state_dict"], fbank_model.spk, x, [target] * 4, f0)
    for i, n in enumerate(lens):
        e = rms(ref[i, 0, :n].numpy() - oref[i, 0, :n].numpy())
        assert e < 1e-5, (i, e)


@pytest.mark.parametrize("B,n", [(1, 1600), (1, 3200), (2, 6400), (3, 80001), (1, 200000), (33, 48000), (64, 16000)],
                         ids=lambda v: str(v))
def test_extreme_sizes_match_oracle_or_raise_like_the_reference(fbank_model, fbank_tag_state, B, n):
    """sizes far off the 5 s / batch-of-32 grid (was tests/diagnostics/robust_sizes.py): 0.1 s utterances, 12.5 s, 33 and
    64 utterances, n = 80001.  Small cases are compared with the CPU oracle on every utterance, the large batches on
    three of them (slices of a batch are the batch: test_full_size_*); nothing may be non-finite"""
    from oracle import convert as oconv
    from satools_amd import synthetic
    wav = synthetic.harm_batch(list(range(B)), n)
    tg = synthetic.targets(fbank_model.spk, list(range(B)))
    try:
        f0 = _oracle_f0(wav)
    except RuntimeError:
        with pytest.raises(RuntimeError):       # the reference fails when no frame is voiced (medfilt / unfold on an empty track)
            fbank_model.convert(wav.to(DEV), target=tg if B > 1 else tg[0])
        return
    y = fbank_model.convert(wav.to(DEV), target=tg if B > 1 else tg[0])
    assert torch.isfinite(y).all()
    state, _ = fbank_tag_state
    if B <= 3:
        ref = oconv.convert_fbank(state["base_model_state_dict"], fbank_model.spk, wav, tg if B > 1 else tg[0], f0)
        assert y.shape == ref.shape
        assert rms(y.cpu().numpy() - ref.numpy()) < 1e-5
    else:
        # the batch-coupled F0 normalisation needs the whole batch: the oracle's _forward on the GPU path's own
        # bottleneck features is not the point here; compare the F0 tracks (all utterances) and three waveforms
        assert torch.equal(fbank_model.get_f0(wav.to(DEV)).cpu()[:, 1:], f0[:, 1:])
        ref = oconv.convert_fbank(state["base_model_state_dict"], fbank_model.spk, wav, tg, f0)
        for i in (0, B // 2, B - 1):
            assert rms(y[i].cpu().numpy() - ref[i].numpy()) < 1e-5, i


def test_sharded_job_runs_on_rccl_in_a_child_process():
    """the multi-GPU path of bench.py (satools_amd.dist: contiguous shards, fixed batches, ONE all_gather_into_tensor over
    RCCL) with a process group of one rank, in a CHILD process (this process has initialised the GPU and is never
    re-executed): the ranks RCCL saw, the gathered job = the shard, both tags, float and PCM16 gathers"""
    env = dict(os.environ, SAT_BENCH_FORCE_PG="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", LOCAL_RANK="0",
               WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    # (--headline-only: the fbank tag of configs[1]; with --full and without it the wav2vec2 tag of BASELINE configs[4] runs first
    # through the same code and its line goes to stderr as CONFIG_LINE)
    # (round 5: the exchange is issued in chunks of --gather-chunk batches on a communication stream while the shard is computed;
    # 0 = the single all_gather_into_tensor at the end, which every run also performs afterwards as the checked reference)
    for extra in (["--headline-only", "--gather-chunk", "1"], ["--full", "--gather", "pcm16"], ["--headline-only", "--gather-chunk", "0"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--no-cpu-baseline"] + extra, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])]
        lines += [json.loads(l[len("CONFIG_LINE "):]) for l in r.stderr.splitlines() if l.startswith("CONFIG_LINE ")]
        assert len(lines) == (1 if "--headline-only" in extra else 2)
        for line in lines:
            cfg = line["config"]
            assert cfg["ranks_seen_by_rccl"] == [0], cfg
            assert cfg["all_gather_ms"] > 0.0
            assert cfg["gathered_equals_shard"] is True and cfg["chunked_equals_single_collective"] is True, cfg
            assert len(cfg["compute_ms_per_rank"]) == 1 and cfg["compute_ms_min_max"][0] > 0.0
            if "--gather-chunk" in extra:
                k = int(extra[extra.index("--gather-chunk") + 1])
                assert ("2 asynchronous all-gathers" in cfg["all_gather"]) == (k == 1) and ("one all_gather_into_tensor" in cfg["all_gather"]) == (k == 0), cfg["all_gather"]
            assert cfg["gather_dtype"] == ("int16" if "pcm16" in extra else "float32")
            assert cfg["utterances"] == 64 and line["n_gpus"] == 1 and line["value"] > 0 and line["repeats"]["windows"] >= 1
        if len(lines) == 2:
            assert "wav2vec2" in lines[1]["config"]["workload"] and "wav2vec2" not in lines[0]["config"]["workload"]


def test_plain_bench_times_exactly_its_steps_and_dumps_the_last_step(tmp_path):
    """a plain `bench.py` run (no --full): the headline alone in ONE window of exactly --steps steps, no side measurements, and
    --dump-outputs writes the last timed step's convert() output as float32; a second run with the same arguments writes the same"""
    dumps = []
    for i in range(2):
        out = tmp_path / f"dump{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 3 and line["repeats"]["windows"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "roofline" not in line and "cpu_baseline" not in line and "configs" not in line
        assert "CONFIG_LINE" not in r.stderr
        y = np.load(out / "convert_y.npy")
        assert y.dtype == np.float32 and y.shape == (32, 1, 80001) and np.isfinite(y).all() and np.abs(y).max() > 0
        dumps.append(y)
    assert np.array_equal(dumps[0], dumps[1])


@pytest.mark.parametrize("tag", [FBANK_TAG, W2V2_TAG])
def test_frozen_export_round_trip(tmp_path, tag):
    """satools_amd.export_frozen / load_frozen (the analogue of the reference's final.jit, hifigan/model.py:162-171): a
    file of kernel-ready weights loads into the same Net interface without parameters and converts to the same bits"""
    import satools_amd
    from satools_amd import synthetic
    model = satools_amd.load_model("synthetic:" + tag)
    model.to(DEV)
    model.eval()
    wav = synthetic.harm_batch([0, 1], 16000).to(DEV)
    tg = synthetic.targets(model.spk, [4, 5])
    ref = model.convert(wav, target=tg)
    path = str(tmp_path / "final.frozen")
    satools_amd.export_frozen(model, path)
    del model
    torch.cuda.empty_cache()
    fz = satools_amd.load_frozen(path, DEV)
    assert sum(p.numel() for p in fz.parameters()) == 0          # inference-only: no f32 parameters on the device
    assert fz.spk == sorted(set(fz.utt2spk.values()))
    y = fz.convert(wav, target=tg)
    assert torch.equal(y, ref)
    assert torch.equal(fz.get_bn(wav), fz.get_bn(wav)) and fz.get_f0(wav).shape == (2, 50)
    assert fz.eval() is None                                       # the reference's quirk survives
    with pytest.raises(Exception):
        satools_amd.export_frozen(fz, path + "2")                   # a frozen model has nothing left to export from
    assert os.path.getsize(path) < (1.5e9 if "wav2vec2" in tag else 2.0e8)


def _convert_forced_window(model, wav, tg):
    """convert() with the near-tie guard forced to flag and rewrite every utterance (as test_hip_guards.py
    test_convert_patches_near_tie_utterances) -> (y, tie_stats of that call, y of the deferred form, its rewritten rows)"""
    ext = model.bn_extractor
    keep = ext.vq_tie_sigmas
    ext.vq_tie_sigmas, ext.vq_tie_force_patch = 1e6, True
    ext.__dict__.pop("tie_stats", None)
    try:
        y = model.convert(wav, target=tg).clone()
        stats = dict(ext.tie_stats)
        y_def, st = model.convert(wav, target=tg, defer_status=True)
        st.check()
        torch.cuda.synchronize()
        return y, stats, y_def.clone(), st.rows
    finally:
        ext.vq_tie_sigmas, ext.vq_tie_force_patch = keep, False


# 5 s `harm` batches of test_vq_flip_rate_of_the_default_arithmetic whose utterances 3005 (first batch) and 3260, 3274, 3278 (second)
# carry near-ties the fbank tag's default window flags
FROZEN_TIE_BATCHES = (3000, 3256)


def test_frozen_fbank_model_keeps_the_near_tie_guard(tmp_path):
    """A frozen fbank-tag model decides near-tie utterances again like the model it was exported from: the file stores the guard's
    calibration and the exact-f32 packing of the TDNNF stack.  (1) Forced window (every utterance flagged and rewritten): 3 utterances
    decided again, the bits of the unfrozen model's convert(), plain and deferred.  (2) The default window on two 32 x 5 s batches
    (seeds 3000-3031 and 3256-3287: FROZEN_TIE_BATCHES) that carry flagged utterances: the delivered indices are the exact-f32
    kernels' and as many utterances are decided again as on the unfrozen model."""
    import satools_amd
    from satools_amd import synthetic
    model = satools_amd.load_model("synthetic:" + FBANK_TAG)
    model.to(DEV)
    model.eval()
    ext = model.bn_extractor
    wav = synthetic.harm_batch([31, 32, 33], 32000).to(DEV)
    tg = [model.spk[1], model.spk[0], model.spk[2]]
    y_ref, st_ref, _, _ = _convert_forced_window(model, wav, tg)
    assert st_ref["rerun"] == 3, st_ref
    batches = [synthetic.harm_batch(list(range(s, s + 32)), 80000).to(DEV) for s in FROZEN_TIE_BATCHES]
    exact, rerun_ref = [], []
    for w in batches:
        with ext._exact(ext):
            _, (_, idx32, _) = ext.extract_bn(w.clone(), want_aux=True)
        exact.append(idx32.clone())
        ext.__dict__.pop("tie_stats", None)
        idx, _ = ext.vq_indices(w)
        assert torch.equal(idx, idx32)
        rerun_ref.append(ext.tie_stats["rerun"])
    assert sum(rerun_ref) >= 1, rerun_ref          # the set carries near-ties: otherwise this part proves nothing
    path = str(tmp_path / "final.frozen")
    satools_amd.export_frozen(model, path)
    del model, ext
    torch.cuda.empty_cache()
    fz = satools_amd.load_frozen(path, DEV)
    fe = fz.bn_extractor
    y, st, y_def, rows = _convert_forced_window(fz, wav, tg)
    print(f"frozen fbank model, forced window: {st}; default window: {rerun_ref} utterances decided again on the unfrozen model")
    assert st["rerun"] == 3 and st.get("unguarded", 0) == 0, st
    assert torch.equal(y, y_ref)
    assert rows == [0, 1, 2] and torch.equal(y_def, y)
    for w, idx32, n_ref in zip(batches, exact, rerun_ref):
        fe.__dict__.pop("tie_stats", None)
        idx, _ = fe.vq_indices(w)
        assert fe.tie_stats["rerun"] == n_ref, (fe.tie_stats, n_ref)
        assert torch.equal(idx, idx32)
    with fe._exact(fe):                             # the exact-f32 packing really runs under _exact (not the split one again)
        _, (_, idx32_f, _) = fe.extract_bn(batches[0].clone(), want_aux=True)
    assert torch.equal(idx32_f, exact[0])


def test_frozen_wav2vec2_model_guard_with_and_without_the_exact_encoder(tmp_path, caplog):
    """wav2vec2 tag.  Default export (the exact-f32 encoder, ~1.2 GB, left out; the file stays under the 1.5e9 bytes of
    test_frozen_export_round_trip): one warning at load, near-ties still counted — under the forced window every utterance is
    `unguarded`, none decided again — and convert() runs; asking for the exact kernels raises instead of running the split packing.
    Opt-in export (`exact_extractor=True`): the forced window decides all 3 utterances again, to the unfrozen model's bits."""
    import logging

    import satools_amd
    from satools_amd import _lib, synthetic
    model = satools_amd.load_model("synthetic:" + W2V2_TAG)
    model.to(DEV)
    model.eval()
    wav = synthetic.harm_batch([31, 32, 33], 32000).to(DEV)
    tg = [model.spk[1], model.spk[0], model.spk[2]]
    y_ref, st_ref, _, _ = _convert_forced_window(model, wav, tg)
    assert st_ref["rerun"] == 3, st_ref
    p0, p1 = str(tmp_path / "default.frozen"), str(tmp_path / "exact.frozen")
    satools_amd.export_frozen(model, p0)
    satools_amd.export_frozen(model, p1, exact_extractor=True)
    s0, s1 = os.path.getsize(p0), os.path.getsize(p1)
    print(f"frozen wav2vec2 files: default {s0 / 1e9:.3f} GB, with the exact-f32 extractor {s1 / 1e9:.3f} GB")
    assert s0 < 1.5e9 < s1
    del model
    torch.cuda.empty_cache()

    with caplog.at_level(logging.WARNING, logger="satools_amd"):
        fz = satools_amd.load_frozen(p0, DEV)
    warned = [r for r in caplog.records if "near-tie" in r.getMessage()]
    assert len(warned) == 1, [r.getMessage() for r in caplog.records]
    fe = fz.bn_extractor
    y, st, _, rows = _convert_forced_window(fz, wav, tg)
    assert st["unguarded"] == 3 and st["rerun"] == 0 and st["utterances"] == 3, st
    assert rows == [] and y.shape == y_ref.shape and torch.isfinite(y).all()
    with pytest.raises(_lib.SatError):
        with fe._exact(fe):
            fe.extract_bn(wav.clone(), want_aux=True)
    del fz, fe
    torch.cuda.empty_cache()

    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="satools_amd"):
        fz = satools_amd.load_frozen(p1, DEV)
    assert not [r for r in caplog.records if "near-tie" in r.getMessage()]
    y, st, y_def, rows = _convert_forced_window(fz, wav, tg)
    assert st["rerun"] == 3 and st.get("unguarded", 0) == 0, st
    assert torch.equal(y, y_ref)
    assert rows == [0, 1, 2] and torch.equal(y_def, y)


def test_check_precision_guards_against_out_of_range_checkpoints():
    """Net.check_precision(): the load-time guard of the split-f16 arithmetic.  A sane checkpoint passes and keeps its
    kernels; one whose inner activations exceed the f16 range (conv1 of every ResBlock step scaled by 2^18 against its
    conv2 — the same function in exact arithmetic, t1 ~ 2e5 > 65504) is detected and falls back to the exact-f32
    kernels, after which convert() matches the CPU oracle again instead of saturating silently"""
    import warnings
    import satools_amd
    from oracle import convert as oconv
    from satools_amd import synthetic
    model = satools_amd.load_model("synthetic:" + FBANK_TAG)
    model.to(DEV)
    model.eval()
    rep = model.check_precision()
    print("check_precision on the synthetic checkpoint:", rep)
    assert rep["fallback"] == [] and rep["generator"] < 2e-5 and rep["bn_index_agreement"] == 1.0 and rep["bn_extractor"] < 1e-4
    assert model.hifigan.precision in ("f16x3", "f16f8r") and model.bn_extractor.precision == "f16x3"      # kept as loaded
    state, _ = synthetic.checkpoint(FBANK_TAG)
    sd = {k: v.clone() for k, v in state["base_model_state_dict"].items()}
    for k in list(sd):
        if k.startswith("hifigan.resblocks.") and k.endswith("weight_g"):
            sd[k] = sd[k] * (2.0 ** 18 if ".convs1." in k else 2.0 ** -18)
        if k.startswith("hifigan.resblocks.") and ".convs1." in k and k.endswith(".bias"):
            sd[k] = sd[k] * 2.0 ** 18
    model.load_state_dict(sd)
    wav = synthetic.harm_batch([2], 16000)
    f0 = _oracle_f0(wav)
    ref = oconv.convert_fbank(sd, model.spk, wav, model.spk[1], f0)
    bad = rms(model.convert(wav.to(DEV), target=model.spk[1]).cpu().numpy() - ref.numpy())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rep = model.check_precision()
    print("check_precision on the out-of-range checkpoint:", rep, "error before the guard", bad)
    assert "generator" in rep["fallback"] and model.hifigan.precision == "f32" and w
    good = rms(model.convert(wav.to(DEV), target=model.spk[1]).cpu().numpy() - ref.numpy())
    assert bad > 1e-4 and good < 1e-5, (bad, good)


def test_asr_forward_of_a_ragged_utterance_list():
    """TdnnfVqNet.forward_ragged: utterances of 1 s, 2.5 s, 1.7 s and 0.6 s in two batched passes = `forward()` of each
    utterance alone (what the reference's decoder driver feeds, chain/decoder.py:24-39), and the oracle's forward"""
    import satools_amd
    from oracle import tdnnf as otd
    from satools_amd import synthetic
    tag = "bn_tdnnf_600h_vq_48_v1"
    net = satools_amd.load_model("synthetic:" + tag)
    net.to(DEV)
    net.eval()
    lens = [16000, 40000, 27200, 9600]
    wavs = [synthetic.harm_batch([20 + i], n)[0].to(DEV) for i, n in enumerate(lens)]
    keep = [w.clone() for w in wavs]
    got = net.forward_ragged(wavs)
    assert all(torch.equal(a, b) for a, b in zip(wavs, keep))            # inputs untouched
    for i, w in enumerate(wavs):
        c1, x1 = net.forward(w.reshape(1, -1).clone())
        assert got[i][0].shape == c1[0].shape and got[i][1].shape == x1[0].shape, (i, got[i][0].shape, c1.shape)
        # the batch may be served by another tile shape of the same kernels than a single utterance: f32 re-association only
        assert (got[i][0] - c1[0]).abs().max().item() < 2e-5 * max(1.0, c1.abs().max().item()), i
        assert (got[i][1] - x1[0]).abs().max().item() < 2e-5 * max(1.0, x1.abs().max().item()), i
    state, _ = synthetic.checkpoint(tag)
    ref_c, ref_x = otd.forward_fbank(state["base_model_state_dict"], wavs[1].cpu().reshape(1, -1))
    assert rms(got[1][0].cpu().numpy() - ref_c[0].numpy()) < 1e-4 * max(1.0, rms(ref_c[0].numpy()))
    assert rms(got[1][1].cpu().numpy() - ref_x[0].numpy()) < 1e-4 * max(1.0, rms(ref_x[0].numpy()))
