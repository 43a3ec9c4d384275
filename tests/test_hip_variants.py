"""The clean and many-to-one anonymizer configs (sa-toolkit_amd/anonymizer_variants.py) on the GPU against the reference's own runs
(tests/golden/fx_variants.npz, written by tests/golden/make_variant_fixtures.py): short utterances, fbank-based extractors.

Bars, unchanged from the tests of the same arithmetic:
  convert() against the reference waveform      1e-4 RMS   tests/test_hip_parity.py::test_convert_matches_golden and
                                                           tests/test_hip_tags.py::test_convert_without_a_quantiser_matches_the_reference_waveform
  every utterance decided again vs exact f32    3e-6 RMS   tests/test_hip_guards.py::test_convert_patches_near_tie_utterances
The normalised F0 the clean config leaves in the caller's tensor is two correctly rounded float32 operations on the fixture's own
statistics: 3 * 2^-24 * |q| (tests/ref64_geninput.py).  VQ indices are held exactly through the generator's input: its bn rows are
codebook rows, so the recorded last channel and the float64 sums of all 256 channels must agree to the two roundings of the
reference's straight-through form (`_check_input`), which one frame with another index would miss by orders of magnitude.
Needs a real MI355X: run with `-m gpu`."""
import os
import types

import numpy as np
import pytest
import torch

import ref64_geninput as r64
from conftest import rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
VQ, AUG = "bn_tdnnf_600h_vq_48", "bn_tdnnf_600h_aug"
TAGS = {"clean": "clean_hifigan_{}_v1", "m2o": "hifigan_m2o_{}_v1"}
SEED_AWGN = 1234
_MODELS = {}


def _model(kind, asr, spec=""):
    key = (kind, asr, spec)
    if key not in _MODELS:
        import satools_amd
        m = satools_amd.load_model("synthetic:" + TAGS[kind].format(asr), option_args={"f0_transformation": spec} if spec else None)
        m.to(DEV)
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


@pytest.fixture(scope="module")
def fx(gold):
    return gold.npz("fx_variants.npz")


def _run(model, fx, prefix, hand="f0", seed=None):
    """convert() of the case `prefix` with the generator's input captured -> (y, x, the tensor handed over or None)"""
    seen = {}
    h = model.hifigan.register_forward_pre_hook(lambda m, a: seen.update(x=a[0].detach().clone()))
    wav = torch.from_numpy(fx[prefix + "wav"].copy())
    handed = None
    if hand is not None and prefix + hand in fx.files:
        handed = torch.from_numpy(fx[prefix + hand].copy())
        model.set_f0(handed)
    if seed is not None:
        torch.manual_seed(seed)
    try:
        if prefix + "targets" in fx.files:
            y = model.convert(wav.to(DEV), target=[model.spk[int(t)] for t in fx[prefix + "targets"]])
        else:
            y = model.convert(wav.to(DEV))
    finally:
        h.remove()
    return y.cpu(), seen["x"].cpu(), handed


def _check_input(x, fx, prefix, exact_bn, f0_tol):
    c_bn = 256
    if exact_bn:
        # the VQ decision, frame by frame.  The reference hands on `inputs + (quantized - inputs)` (chain/nn.py:459), two roundings that depend on
        # its own inputs: each element lies within 2^-23 (|q| + |inputs|) <= 2^-22 max|x| of the codebook value, a channel's sum within T times
        # that.  A frame with another index moves 256 channels by the distance of two codebook rows, of order 1.
        top = float(np.abs(fx[prefix + "x_bn_last"]).max())
        tol = 2.0 ** -22 * max(top, float(x[:, :c_bn].abs().max()))
        assert np.abs(x[:, c_bn - 1].numpy() - fx[prefix + "x_bn_last"]).max() <= tol, prefix
        sums = x.double().sum(dim=2).numpy()
        assert np.abs(sums[:, :c_bn] - fx[prefix + "x_sums"][:, :c_bn]).max() <= x.shape[2] * tol, prefix
    else:
        assert np.abs(x[:, c_bn - 1].numpy() - fx[prefix + "x_bn_last"]).max() < 1e-4, prefix
    want = fx[prefix + "x_f0"].astype(np.float64)
    assert np.all(np.abs(x[:, c_bn].double().numpy() - want) <= f0_tol(want)), (prefix, float(np.abs(x[:, c_bn].double().numpy() - want).max()))
    if prefix + "x_spk" in fx.files:
        assert np.array_equal(x[:, c_bn + 1:].numpy(), fx[prefix + "x_spk"].astype(np.float32)), prefix
    else:
        assert x.shape[1] == c_bn + 1


_NORM = lambda q: r64.NORM_BOUND * np.abs(q)          # noqa: E731


@pytest.mark.parametrize("asr,case", [(VQ, "b1"), (VQ, "b2_two_targets"), (AUG, "b2_two_targets")])
def test_clean_convert_matches_the_reference(fx, asr, case):
    model = _model("clean", asr)
    prefix = f"clean/{asr}/{case}/"
    y, x, handed = _run(model, fx, prefix)
    want = fx[prefix + "y"]
    err = rms(y.numpy() - want)
    print(f"{prefix} RMS error vs reference {err:.2e} (signal {rms(want):.3f})")
    assert y.shape == want.shape and err < 1e-4
    _check_input(x, fx, prefix, asr == VQ, _NORM)
    # the caller's tensor holds the normalised values afterwards
    after = fx[prefix + "f0_after"].astype(np.float64)
    assert np.all(np.abs(handed.double().numpy() - after) <= _NORM(after)) and not handed[torch.from_numpy(fx[prefix + "f0"]) == 0].any()
    assert model.f0 is None


def test_clean_normalises_the_whole_batch_with_the_first_targets_statistics(fx):
    prefix = f"clean/{VQ}/b2_two_targets/"
    model = _model("clean", VQ)
    _, x, _ = _run(model, fx, prefix)
    t = [int(v) for v in fx[prefix + "targets"]]
    table, f0 = fx["clean/table"], fx[prefix + "f0"]
    assert t[0] != t[1] and not np.array_equal(table[t[0]], table[t[1]])
    idx = r64.interp_index(x.shape[2], f0.shape[1])
    first = r64.normalise(f0, table[t[0], 0], table[t[0], 1])[:, idx]
    own = r64.normalise(f0[1], table[t[1], 0], table[t[1], 1])[idx]
    got = x[:, 256].double().numpy()
    assert np.all(np.abs(got - first) <= _NORM(first))                            # both rows: the first target's mean and std
    assert np.abs(got[1] - own).max() > 0.1                                       # not row 1's own target's
    assert np.array_equal(x[:, 257:].argmax(dim=1).numpy(), np.repeat(np.asarray(t)[:, None], x.shape[2], axis=1))   # the one-hots are per row


def test_clean_refuses_a_target_without_statistics(fx):
    import satools_amd
    from satools_amd import synthetic
    model = satools_amd.load_model("synthetic:" + TAGS["clean"].format(VQ))
    k = int(fx["clean/missing_speaker"])
    sd = model.state_dict()
    sd["f0_norm.model_state_buffer"] = synthetic.speaker_cmvn_buffer(len(model.spk), 0, skip=(k,))
    model.load_state_dict(sd)
    model.to(DEV)
    model.eval()
    wav = synthetic.harm_batch([2], 9600)
    model.set_f0(torch.from_numpy(fx[f"clean/{VQ}/quant_16_awgn_2/f0"].copy()))
    assert str(fx["clean/missing_type"]) == "RuntimeError"
    with pytest.raises(RuntimeError) as e:
        model.convert(wav.to(DEV), target=[model.spk[k]])
    assert type(e.value) is RuntimeError and str(e.value) == str(fx["clean/missing_message"])
    model.set_f0(torch.from_numpy(fx[f"clean/{VQ}/quant_16_awgn_2/f0"].copy()))
    assert model.convert(wav.to(DEV), target=[model.spk[k + 1]]).shape == (1, 9601)       # its neighbour has them


@pytest.mark.parametrize("asr,case", [(VQ, "b1"), (AUG, "b1")])
def test_m2o_convert_matches_the_reference(fx, asr, case):
    model = _model("m2o", asr)
    prefix = f"m2o/{asr}/{case}/"
    y, x, _ = _run(model, fx, prefix)
    want = fx[prefix + "y"]
    err = rms(y.numpy() - want)
    print(f"{prefix} RMS error vs reference {err:.2e} (signal {rms(want):.3f})")
    assert y.shape == want.shape and err < 1e-4 and not hasattr(model, "spk")
    # batch-coupled statistics: the reduction's order differs from torch's, so the F0 row is held to the existing path's own level
    # (tests/test_hip_small_kernels.py: mean and std to a few 1e-7 relative), 1e-5 absolute on values of order 1
    _check_input(x, fx, prefix, asr == VQ, lambda q: 1e-5 + 0 * q)


def test_m2o_never_reads_a_track_handed_over_by_set_f0(fx):
    model = _model("m2o", VQ)
    prefix = f"m2o/{VQ}/b2_set_f0_ignored/"
    y, x, handed = _run(model, fx, prefix)
    assert rms(y.numpy() - fx[prefix + "y"]) < 1e-4 and y.shape == fx[prefix + "y"].shape
    assert np.array_equal(handed.numpy(), fx[prefix + "f0_after"]) and bool((handed == 123.0).all())
    model.f0 = None
    y2, x2, _ = _run(model, fx, prefix, hand=None)
    assert torch.equal(y2, y) and torch.equal(x2, x)
    _check_input(x, fx, prefix, True, lambda q: 1e-5 + 0 * q)


@pytest.mark.parametrize("kind", ["clean", "m2o"])
def test_quant_and_awgn_run_inside_the_fused_launch(fx, kind):
    model = _model(kind, VQ, "quant_16_awgn_2")
    prefix = f"{kind}/{VQ}/quant_16_awgn_2/"
    y, x, _ = _run(model, fx, prefix, seed=SEED_AWGN)
    err = rms(y.numpy() - fx[prefix + "y"])
    print(f"{prefix} RMS error vs reference {err:.2e}")
    assert err < 1e-4
    # quantised values plus the seeded noise: one rounded float32 sum on equal operands (clean), on operands 1e-5 apart at most (m2o) unless a
    # value sat on a quantiser edge, which would show as a step of 1 / 16
    _check_input(x, fx, prefix, True, (lambda q: 0 * q) if kind == "clean" else (lambda q: 1e-5 + 0 * q))


def test_mean_reverv_takes_the_existing_calls_and_gives_the_fused_input_transformed(fx):
    from satools_amd import _lib
    prefix = f"clean/{VQ}/b1/"
    plain, rev = _model("clean", VQ), _model("clean", VQ, "mean-reverv_0.5:5")
    _, x_plain, norm = _run(plain, fx, prefix)
    _, x_rev, norm_rev = _run(rev, fx, prefix)
    assert torch.equal(norm, norm_rev)                                            # both leave the same normalised track with the caller
    src = norm.reshape(-1).to(DEV).contiguous()
    out = torch.empty_like(src)
    _lib.check(_lib.lib().sat_f0_mean_reversion_f32(_lib.ptr(src), _lib.ptr(out), src.numel(), 0.5, 5, _lib.stream()), "sat_f0_mean_reversion_f32")
    idx = torch.from_numpy(r64.interp_index(x_plain.shape[2], src.numel()))
    want = x_plain.clone()
    want[0, 256] = out.cpu()[idx]
    assert torch.equal(x_rev, want) and not torch.equal(x_rev, x_plain)


@pytest.mark.parametrize("kind", ["clean", "m2o"])
def test_every_utterance_decided_again_gives_the_plain_runs_output(kind):
    from satools_amd import synthetic
    model = _model(kind, VQ)
    ext = model.bn_extractor
    wav = synthetic.harm_batch([31, 32], 12800).to(DEV)
    kw = {"target": [model.spk[1], model.spk[0]]} if kind == "clean" else {}
    keep = ext.vq_tie_sigmas
    try:
        ext.vq_tie_sigmas = 0.0
        y_plain = model.convert(wav, **kw).clone()
        ext.vq_tie_sigmas, ext.vq_tie_force_patch = 1e6, True
        ext.__dict__.pop("tie_stats", None)
        y_all = model.convert(wav, **kw).clone()
        assert ext.tie_stats["rerun"] == 2 and ext.tie_stats["changed"] == 2, ext.tie_stats
        y_def, st = model.convert(wav, defer_status=True, **kw)
        st.check()
        torch.cuda.synchronize()
        assert st.rows == [0, 1] and torch.equal(y_def, y_all)
        ext.vq_tie_force_patch = False
        ext.__dict__.pop("tie_stats", None)
        y_cmp = model.convert(wav, **kw).clone()                                    # decided again, rewritten only where an index changed
        assert ext.tie_stats["rerun"] == 2 and (ext.tie_stats["changed"] > 0 or torch.equal(y_cmp, y_plain)), ext.tie_stats
        ext.vq_tie_sigmas = 0.0
        with ext._exact(ext):
            y_exact = model.convert(wav, **kw).clone()
    finally:
        ext.vq_tie_sigmas, ext.vq_tie_force_patch = keep, False
    e_all = rms((y_all - y_exact).cpu().numpy())
    print(f"{kind}: every utterance decided again vs the exact-f32 extractor {e_all:.2e}; plain run {rms((y_plain - y_exact).cpu().numpy()):.2e}")
    assert e_all < 3e-6, e_all


def test_check_precision_runs_on_both_nets():
    for kind in ("clean", "m2o"):
        rep = _model(kind, VQ).check_precision()
        print(kind, rep)
        assert rep["fallback"] == [] and rep["generator"] < 1e-3


def test_frozen_export_is_refused_by_name(tmp_path):
    import satools_amd
    from satools_amd import _lib
    for kind, cfg in (("clean", "hifigan_clean.py"), ("m2o", "hifigan_m2o.py")):
        with pytest.raises(_lib.SatError, match="frozen export is not built for the 'local/tuning/" + cfg):
            satools_amd.export_frozen(_model(kind, VQ), str(tmp_path / "x.sat"))


@pytest.mark.parametrize("kind", ["clean", "m2o"])
def test_the_batch_job_writes_converts_samples(tmp_path, kind):
    from pipeline_toy import read_wav, write_wav
    from satools_amd import pipeline as pl
    from satools_amd import synthetic
    data = str(tmp_path / "data" / "toy")
    os.makedirs(os.path.join(data, "clear"))
    scp_lines, u2s = [], []
    for i in range(3):
        path = os.path.join(data, "clear", f"utt{i:02d}.wav")
        write_wav(path, synthetic.harm_batch([i], 9600)[0].numpy().astype(np.float64))
        scp_lines.append(f"utt{i:02d} {path}\n")
        u2s.append(f"utt{i:02d} src{i % 2}\n")
    open(os.path.join(data, "wav.scp"), "w").writelines(scp_lines)
    open(os.path.join(data, "utt2spk"), "w").writelines(u2s)
    model = _model(kind, VQ)
    assert not hasattr(model, "convert_padded")
    with pytest.raises(AttributeError, match="convert_padded is not built for the 'local/tuning/hifigan_" + kind):
        model.convert_padded
    target = model.spk[5] if kind == "clean" else "?"
    settings = types.SimpleNamespace(model="-", f0_modification="", target_constant_spkid=target, results_dir="wav", batch_size=3,
                                     data_loader_nj=2, new_datadir_suffix="_anon", device="cuda")
    scp = pl.read_wav_scp(os.path.join(data, "wav.scp"))
    assert pl.process_data(data, "constant" if kind == "clean" else "none", scp, settings, model=model) == 3
    wavs = torch.cat([pl.load_wav_from_scp(scp[f"utt{i:02d}"])[0] for i in range(3)]).to("cuda")
    if kind == "clean":
        model.set_f0(model.get_f0_ragged(wavs, torch.tensor([9600] * 3)))           # what the job hands over: per-utterance tracks
        ref = model.convert(wavs, target=[target] * 3).cpu()
    else:
        ref = model.convert(wavs).cpu()
    for i in range(3):
        got, sr = read_wav(os.path.join(data + "_anon", "wav", f"utt{i:02d}.wav"))
        exp = np.clip(np.rint(ref[i, 0, :9600].numpy().astype(np.float64) * 32768), -32768, 32767).astype(np.int16)
        assert sr == 16000 and got.shape == (9600,) and np.array_equal(got, exp)
