"""The tags beyond the first three through the models, on the HIP path: the nets without a quantiser (`bn_tdnnf_600h_aug`,
`bn_tdnnf_wav2vec2_100h_aug`) and the 256-code VQ (`bn_tdnnf_100h_vq_256`, whose codebook the tiled kernel walks) against the
reference's own outputs (tests/golden/fx_tags.npz, fx_e2e_<name>.npz: make_tag_fixtures.py) and the CPU oracle.
Needs a real MI355X: run with `-m gpu`.

Measured (MI355X; convert() against the reference's waveform, 5 s utterances, RMS, B = 1 / B = 2; signal RMS 0.17 / 0.10).  Without a
quantiser the extractor's arithmetic reaches the generator un-quantised — no code lookup erases it:
    hifigan_bn_tdnnf_600h_aug_v1      f16f8r 2.51e-6 / 2.54e-6   f16x3 1.89e-6 / 1.92e-6   f32 1.69e-6 / 1.70e-6     (bar 1e-4)
    hifigan_bn_tdnnf_100h_vq_256_v1   default arithmetic 2.99e-7 / 3.02e-7                                          (bar 1e-4)
The guard at 256 codes on the 536-utterance set: 0 flips in 158 000 frames, 17 utterances (3.2 %) decided again, 5 of them changed
(the raw split-f16 arithmetic: 5 flips = 32 per million frames)."""
import pytest
import torch

from conftest import rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
AUG_TAG = "hifigan_bn_tdnnf_600h_aug_v1"
VQ256_TAG = "hifigan_bn_tdnnf_100h_vq_256_v1"
W2V2_AUG_TAG = "hifigan_bn_tdnnf_wav2vec2_100h_aug_v1"


def _model(tag):
    import satools_amd
    m = satools_amd.load_model("synthetic:" + tag)
    m.to(DEV)
    m.eval()
    return m


@pytest.fixture(scope="module")
def aug():
    return _model(AUG_TAG)


@pytest.fixture(scope="module")
def vq256():
    return _model(VQ256_TAG)


@pytest.fixture(scope="module")
def aug_state():
    from satools_amd import synthetic
    return synthetic.checkpoint(AUG_TAG)[0]


class _arith:
    """context: extractor / generator arithmetic of a model, restored afterwards"""

    def __init__(self, model, ext=None, gen=None):
        self.model, self.ext, self.gen = model, ext, gen

    def __enter__(self):
        e, g = self.model.bn_extractor, self.model.hifigan
        self.keep = ({k: getattr(e, k) for k in e._precision_keys()}, g.precision)
        if self.ext is not None:
            for k in self.keep[0]:
                setattr(e, k, self.ext)
        if self.gen is not None:
            g.precision = self.gen
            g.invalidate()
        if self.gen == "f16f8r":            # (batches of 1 - 2 utterances are below the ring kernel's default dispatch: this handle runs
            g.set_force_f8(1)               # the 8-bit cross terms at every size, as check_precision does)

    def __exit__(self, *a):
        e, g = self.model.bn_extractor, self.model.hifigan
        if self.gen == "f16f8r":
            g.set_force_f8(0)
        for k, v in self.keep[0].items():
            setattr(e, k, v)
        g.precision = self.keep[1]
        g.invalidate()


# ---- the net without a quantiser, fbank front end ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_extract_bn_without_a_quantiser_matches_reference_and_oracle(aug, aug_state, gold, precision):
    """extract_bn = the 256-dim output of tdnnfs[-2]'s linearB (tdnnf.py:157-177): the tensor the VQ tag's test holds to 2e-4 before
    its quantiser, here the result itself; no guard, no indices"""
    from oracle import convert as oconv
    from oracle import tdnnf as otd
    from satools_amd import _lib, synthetic
    fx = gold.npz("fx_tags.npz")
    asr, _ = oconv.split_state_dict(aug_state["base_model_state_dict"])
    wav = synthetic.harm_batch([0, 1], 80000)
    ref = otd.extract_bn_fbank(asr, wav)
    ext = aug.bn_extractor
    with _arith(aug, ext=precision):
        bn = ext.extract_bn(wav.clone().to(DEV))
        bn_aux, aux = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
        short = ext.extract_bn(synthetic.harm_batch([0], 8000).to(DEV))
        w2 = wav.clone().to(DEV)
        out = aug.get_bn(w2)
        pair = aug.get_bn(w2, defer_ties=True)
    assert aux is None and torch.equal(bn, bn_aux)
    assert bn.shape == ref.shape == (2, 250, 256)
    e_or = float((bn.cpu() - ref).abs().max())
    e_fx = float((bn.cpu().permute(0, 2, 1)[:, ::8, :] - torch.from_numpy(fx["bn_tdnnf_600h_aug/harm01_80000/bn_sub"])).abs().max())
    e_short = float((short.cpu().permute(0, 2, 1) - torch.from_numpy(fx["bn_tdnnf_600h_aug/harm0_8000/bn"])).abs().max())
    print(f"bn_tdnnf_600h_aug {precision}: max abs error vs oracle {e_or:.2e}, vs reference {e_fx:.2e} (2 x 5 s), {e_short:.2e} (0.5 s)")
    assert e_or < 2e-4 and e_fx < 2e-4 and e_short < 2e-4
    assert out.shape == (2, 256, 250) and torch.equal(w2.cpu(), wav)          # input untouched
    assert torch.equal(out, bn.permute(0, 2, 1))
    assert isinstance(pair, tuple) and pair[1] is None and torch.equal(pair[0], out)
    assert ext._tie_guard(torch.device(DEV)) is None
    st = ext.__dict__.get("tie_stats")
    assert st is None or not any(st.values())
    for fn in (ext.vq_indices, ext.vq_flip_report):
        with pytest.raises(_lib.SatError, match="no VQ bottleneck"):
            fn(wav.to(DEV))


def test_bottleneck_without_a_quantiser_is_read_from_planes_only(aug):
    """split-f16 mode: the layer below the bottleneck writes no f32 output and the bottleneck's linearB runs as its own conv on the
    planes (its plan record: `reads_f32` False) — no launch more than the VQ tag makes before its quantiser, and the result within
    the split-f16 error of the f32 hand-over"""
    from satools_amd import synthetic
    ext = aug.bn_extractor
    layers = ext._stack_layers()
    ext._prepare(torch.device(DEV))
    assert ext.precision == "f16x3" and ext.tdnnf_planes_only
    plan = [p for _, _, p in ext._planned(False)]
    assert len(plan) == len(layers) and plan[-1].bottleneck_only and plan[-1].planes_in and not plan[-1].reads_f32
    assert plan[-2].form == "one_call" and plan[-2].planes_in and plan[-2].z_planes and plan[-2].planes_out and plan[-2].skip_f32
    wav = synthetic.harm_batch([3, 4, 5], 80000).to(DEV)
    keep = ext.tdnnf_planes_only
    try:
        a = ext.extract_bn(wav.clone()).clone()
        ext.tdnnf_planes_only = False
        b = ext.extract_bn(wav.clone()).clone()
    finally:
        ext.tdnnf_planes_only = keep
    err = rms((a - b).cpu().numpy()) / rms(b.cpu().numpy())
    print(f"bottleneck without a quantiser, planes only vs f32 hand-over: {err:.2e} relative RMS")
    assert torch.isfinite(a).all() and err < 1e-5


def _convert_against_fixture(model, gold, name):
    """the cases of test_hip_parity.test_convert_matches_golden on `name`'s reference waveforms -> (RMS error B = 1, B = 2)"""
    from satools_amd import synthetic
    fx, f0fx = gold.npz(f"fx_e2e_{name}.npz"), gold.npz("fx_f0.npz")
    wav = synthetic.harm_batch([0], 80000)
    keep = wav.clone()
    model.set_f0(torch.from_numpy(f0fx["harm0_80000"].copy()))
    y = model.convert(wav.to(DEV), target=model.spk[3])
    assert y.shape == (1, 80001) and y.dtype == torch.float32
    assert torch.equal(wav, keep)
    e1 = rms(y.cpu().numpy() - fx["harm0_80000_str"])
    wav = synthetic.harm_batch([0, 1], 80000)
    model.set_f0(torch.from_numpy(f0fx["harm01_80000_batch"].copy()).to(DEV))
    y = model.convert(wav.to(DEV), target=[model.spk[3], model.spk[10]])
    assert y.shape == (2, 1, 80001)
    e2 = rms(y.cpu().numpy() - fx["harm01_80000_list"])
    assert model.f0 is None
    return e1, e2, rms(fx["harm0_80000_str"])


def test_convert_without_a_quantiser_matches_the_reference_waveform(aug, gold):
    """the un-quantised bottleneck carries the extractor's arithmetic into the generator: the project's bar (1e-4 RMS) in the default
    arithmetic ("f16f8r" generator, split-f16 extractor), in "f16x3" and on the exact-f32 kernels of both — which must come out at
    the level the VQ tags reach (a few 1e-6: f32 re-association through 11 TDNNF layers and the generator)"""
    got = {}
    for name, ext, gen in (("f16f8r", "f16x3", "f16f8r"), ("f16x3", "f16x3", "f16x3"), ("f32", "f32", "f32")):
        with _arith(aug, ext=ext, gen=gen):
            got[name] = _convert_against_fixture(aug, gold, "bn_tdnnf_600h_aug")
            ran = aug.hifigan.last_arithmetic
        e1, e2, sig = got[name]
        assert ran.startswith(gen), (ran, gen)
        print(f"{AUG_TAG} convert RMS error vs reference, {name} (generator ran {ran}): B=1 {e1:.2e} B=2 {e2:.2e} "
              f"(signal RMS {sig:.3f})")
    for name, (e1, e2, _) in got.items():
        assert e1 < 1e-4 and e2 < 1e-4, (name, e1, e2)
    # exact f32 on both sides differs from the reference by f32 re-association alone: the 1e-5 that test_convert_ragged_sizes_match_oracle
    # holds the VQ tag to against the oracle
    assert max(got["f32"][:2]) < 1e-5


@pytest.mark.parametrize("shape", [(1, 4800), (3, 16123), (2, 31999), (5, 9600)], ids=lambda s: f"B{s[0]}xn{s[1]}")
def test_convert_without_a_quantiser_ragged_sizes_match_oracle(aug, aug_state, shape):
    from oracle import convert as oconv
    from oracle import yaapt as oyaapt
    from satools_amd import synthetic
    B, n = shape
    wav = synthetic.harm_batch(list(range(B)), n)
    tg = synthetic.targets(aug.spk, list(range(B)))
    nt = torch.get_num_threads()
    torch.set_num_threads(1)          # the reference's own YAAPT setting (frame 0 is thread-count dependent in torch)
    try:
        f0 = oyaapt.yaapt(wav, {"frame_length": 35.0, "frame_space": 20.0, "nccf_thresh1": 0.25, "tda_frame_length": 25.0})
    finally:
        torch.set_num_threads(nt)
    ref = oconv.convert_fbank(aug_state["base_model_state_dict"], aug.spk, wav, tg if B > 1 else tg[0], f0)
    y = aug.convert(wav.to(DEV), target=tg if B > 1 else tg[0])
    assert y.shape == ref.shape
    err = rms(y.cpu().numpy() - ref.numpy())
    print(f"{AUG_TAG} B={B} n={n}: out {tuple(y.shape)}, RMS error vs oracle {err:.2e}")
    assert err < 1e-4


def test_check_precision_without_a_quantiser(aug):
    """the load-time precision guard: extractor figures without indices or a flip report, nothing falls back"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rep = aug.check_precision()
    print("check_precision,", AUG_TAG, rep)
    assert rep["fallback"] == [] and 0 < rep["bn_extractor"] < 1e-4 and rep["generator"] < 1e-3
    assert "bn_index_agreement" not in rep and "bn_index_flips" not in rep
    assert aug.bn_extractor.precision == "f16x3"


# ---- the net without a quantiser, wav2vec2 front end --------------------------------------------------------------------------
def test_wav2vec2_extract_bn_without_a_quantiser_matches_reference_fixture(gold):
    from satools_amd import synthetic
    fx = gold.npz("fx_tags.npz")
    model = _model(W2V2_AUG_TAG)
    ext = model.bn_extractor
    wav = synthetic.harm_batch([0, 1], 16000)
    bn = ext.extract_bn(wav.clone().to(DEV))
    assert bn.shape == (2, 50, 256)
    ref = torch.from_numpy(fx["bn_tdnnf_wav2vec2_100h_aug/harm01_16000/bn"]).permute(0, 2, 1)
    err = float((bn.cpu() - ref).abs().max())
    print(f"bn_tdnnf_wav2vec2_100h_aug: max abs error vs reference {err:.2e}")
    assert err < 5e-4
    out, fix = model.get_bn(wav.to(DEV), defer_ties=True)
    assert out.shape == (2, 256, 50) and fix is None and ext._tie_guard(torch.device(DEV)) is None
    y = model.convert(wav.to(DEV), target=[model.spk[3], model.spk[10]])
    assert y.shape[:2] == (2, 1) and torch.isfinite(y).all()


# ---- 256 codes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_extract_bn_256_codes_matches_reference_and_oracle(vq256, gold, precision):
    """indices equal to the reference's on every frame whose reference margin exceeds 5e-3 (at most 1 % of the frames fall below)"""
    from oracle import convert as oconv
    from oracle import tdnnf as otd
    from satools_amd import _lib, synthetic
    fx = gold.npz("fx_tags.npz")
    state = synthetic.checkpoint(VQ256_TAG)[0]
    asr, _ = oconv.split_state_dict(state["base_model_state_dict"])
    ext = vq256.bn_extractor
    for name, seeds in (("harm01_80000", [0, 1]), ("harm3to10_80000", list(range(3, 11)))):
        wav = synthetic.harm_batch(seeds, 80000)
        with _arith(vq256, ext=precision):
            bn, (z, idx, dist) = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
            assert "vq_tiled_kernel" in _lib.lib().sat_last_dispatch_name().decode()       # the quantiser is the stack's last launch
            delivered, _ = ext.vq_indices(wav.to(DEV))
        assert dist.shape == (len(seeds), 250, 256)
        margin = torch.from_numpy(fx[f"bn_tdnnf_100h_vq_256/{name}/margin"])
        sure = margin > 5e-3
        assert float((~sure).float().mean()) <= 0.01
        ref_idx = torch.from_numpy(fx[f"bn_tdnnf_100h_vq_256/{name}/idx"]).long()
        agree = idx.cpu().long() == ref_idx
        agree_d = delivered.cpu().long() == ref_idx
        print(f"bn_tdnnf_100h_vq_256 {precision} {name}: {int((~sure).sum())} of {sure.numel()} frames under the margin; indices differing from the "
              f"reference: raw {int((~agree).sum())}, delivered {int((~agree_d).sum())}; {len(set(ref_idx.flatten().tolist()))} codes in use")
        assert agree[sure].all() and agree_d[sure].all()
        if name == "harm01_80000":
            aux = {}
            ref = otd.extract_bn_fbank(asr, wav, aux=aux)
            assert (z.cpu().permute(0, 2, 1) - aux["z"]).abs().max() < 2e-4
            assert (bn.cpu() - ref)[agree & (idx.cpu().long() == aux["idx"])].abs().max() < 2e-4
            sub = torch.from_numpy(fx[f"bn_tdnnf_100h_vq_256/{name}/bn_sub"]).permute(0, 2, 1)          # [2, 250, 32]
            assert (bn.cpu()[:, :, ::8] - sub)[agree].abs().max() < 2e-4


def test_near_tie_guard_at_256_codes_delivers_the_exact_indices(vq256):
    """the delivered indices (`vq_indices`: split-f16 arithmetic, near-ties counted by sat_vq_argmin_gather_tiled_tie_f32, their
    utterances decided again) equal those of the exact-f32 setting on EVERY frame of 512 utterances of 5 s, 16 of 20 s and 8 of 35 s
    (the set of test_hip_robust.test_vq_flip_rate_of_the_default_arithmetic).  Printed, not asserted: the share decided again."""
    from satools_amd import synthetic
    from test_hip_robust import _long_batch
    ext = vq256.bn_extractor
    assert ext.precision == "f16x3" and ext.vq_tie_sigmas > 0
    tot = {"frames": 0, "flips": 0, "raw_flips": 0, "utterances": 0, "rerun": 0, "changed": 0}
    sets = [("5 s", [synthetic.harm_batch(list(range(3000 + 32 * i, 3032 + 32 * i)), 80000) for i in range(16)]),
            ("20 s", [_long_batch(list(range(4000 + 4 * i, 4004 + 4 * i)), 20 * 16000) for i in range(4)]),
            ("35 s", [_long_batch(list(range(5000 + 2 * i, 5002 + 2 * i)), 35 * 16000) for i in range(4)])]
    for name, batches in sets:
        for wav in batches:
            wd = wav.to(DEV)
            ext.__dict__.pop("tie_stats", None)
            idx, rows = ext.vq_indices(wd)
            _, (_, idx_raw, _) = ext.extract_bn(wd.clone(), want_aux=True)
            with ext._exact(ext):
                _, (_, idx32, _) = ext.extract_bn(wd.clone(), want_aux=True)
            tot["frames"] += idx.numel()
            tot["flips"] += int((idx != idx32).sum())
            tot["raw_flips"] += int((idx_raw != idx32).sum())
            tot["utterances"] += wd.shape[0]
            tot["rerun"] += ext.tie_stats["rerun"]
            tot["changed"] += len(rows)
    print(f"VQ indices at 256 codes: {tot['flips']} flips in {tot['frames']} frames; {tot['rerun']} of {tot['utterances']} utterances decided again "
          f"({100.0 * tot['rerun'] / tot['utterances']:.1f} %), {tot['changed']} changed; the raw arithmetic: {tot['raw_flips']} flips = "
          f"{1e6 * tot['raw_flips'] / tot['frames']:.0f} per million (window {ext.vq_tie_sigmas} sigma, sigma_rel {ext._tie[2]:.2e})")
    assert tuple(ext._tie[1].shape) == (256, 256)
    assert tot["flips"] == 0, tot


def test_convert_256_codes_matches_the_reference_waveform(vq256, gold):
    e1, e2, sig = _convert_against_fixture(vq256, gold, "bn_tdnnf_100h_vq_256")
    print(f"{VQ256_TAG} convert RMS error vs reference: B=1 {e1:.2e} B=2 {e2:.2e} (signal RMS {sig:.3f})")
    assert e1 < 1e-4 and e2 < 1e-4


# ---- frozen files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [AUG_TAG, VQ256_TAG])
def test_frozen_round_trip_of_the_new_tags(tmp_path, tag, caplog):
    """export_frozen / load_frozen: the same convert() bits as the live model; the 256-code file carries the guard (pair table
    [256, 256], the exact-f32 packing), the file of the net without a quantiser neither, and loads without a warning"""
    import logging
    import satools_amd
    from satools_amd import synthetic
    model = _model(tag)
    wav = synthetic.harm_batch([0, 1], 16000).to(DEV)
    tg = synthetic.targets(model.spk, [4, 5])
    ref = model.convert(wav, target=tg)
    big = synthetic.harm_batch(list(range(3000, 3032)), 80000).to(DEV)
    has_vq = "vq" in tag
    if has_vq:
        ext = model.bn_extractor
        with ext._exact(ext):
            _, (_, idx32, _) = ext.extract_bn(big.clone(), want_aux=True)
        idx_live, _ = ext.vq_indices(big)
        assert torch.equal(idx_live, idx32)
    path = str(tmp_path / "final.frozen")
    satools_amd.export_frozen(model, path)
    del model
    torch.cuda.empty_cache()
    blob = torch.load(path, weights_only=True, map_location="cpu")
    with caplog.at_level(logging.WARNING, logger="satools_amd"):
        fz = satools_amd.load_frozen(path, DEV)
    assert not [r for r in caplog.records if "exact-f32" in r.getMessage()]
    assert sum(p.numel() for p in fz.parameters()) == 0
    assert torch.equal(fz.convert(wav, target=tg), ref)
    fe = fz.bn_extractor
    if has_vq:
        assert tuple(blob["extractor"]["tie"]["pair"]["__t__"].shape) == (256, 256) and "cache" in blob["extractor"]["exact"]
        pair, scale = fe._tie_guard(torch.device(DEV))
        assert tuple(pair.shape) == (256, 256) and scale > 0 and fe._exact_stored()
        fe.__dict__.pop("tie_stats", None)
        idx, _ = fe.vq_indices(big)
        assert torch.equal(idx, idx32) and fe.tie_stats.get("unguarded", 0) == 0
        print(f"frozen {tag}: {fe.tie_stats} on 32 x 5 s")
    else:
        assert blob["extractor"]["tie"] is None and "exact" not in blob["extractor"]
        assert fe._tie_guard(torch.device(DEV)) is None
        y, st = fz.convert(wav, target=tg, defer_status=True)
        st.check()
        assert torch.equal(y, ref) and not (fe.__dict__.get("tie_stats") or {}).get("unguarded", 0)
