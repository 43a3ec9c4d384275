"""tests/ref64.py — the float64 references the small-kernel tests (test_hip_small_kernels.py) compare against — pinned on the CPU
against the reference's own outputs (tests/golden) and the CPU oracle, so that they cannot drift.

Every bar is the error of float32 arithmetic against float64, measured here: the same formula is evaluated in float32 torch on the
CPU (ref64.in_float32()), and twice its largest deviation from the float64 result is the bar for the reference's float32 output.
The measured figures stand beside the asserts.  CPU only."""
import numpy as np
import torch
import torch.nn.functional as F

import ref64
from oracle import f0 as of0
from oracle import melspec as omel
from oracle import xvector as ox
from satools_amd import synthetic


def _bar(fn, *args):
    """(float64 result, 2 x max |float32 evaluation - float64 result|) of one ref64 formula"""
    want = fn(*args)
    with ref64.in_float32():
        low = fn(*args)
    assert low.dtype == torch.float32 and want.dtype == torch.float64
    return want, 2.0 * float((low.double() - want).abs().max())


def _front_end(wav):
    window, fb = torch.hann_window(400, periodic=True), omel.melscale_fbanks().t().contiguous()
    return ref64.instance_norm(ref64.logmel(wav, window, fb, 0.97))[0]


def test_melspec_then_instance_norm_is_the_reference_front_end(gold):
    fx = gold.npz("fx_xvector.npz")
    for tag, seed, n in (("harm0_16000", 0, 16000), ("harm3_48000", 3, 48000), ("harm7_24123", 7, 24123)):
        want, bar = _bar(_front_end, synthetic.harm_batch([seed], n))
        ref = torch.from_numpy(fx[tag + "/feats"]).double()
        err = float((want - ref).abs().max())
        print(f"front end {tag}: |ref64 - reference| = {err:.3e}, bar (2 x float32 error) = {bar:.3e}")
        assert want.shape == ref.shape
        assert err <= bar, (tag, err, bar)          # measured: err 7.7e-6 .. 1.1e-5 against bars 1.4e-5 .. 2.2e-5
        # ... and the oracle's own front end (torch.stft in float32) sits inside the same bar
        assert float((ox.front_end(synthetic.harm_batch([seed], n)).double() - want).abs().max()) <= bar


def test_f0_normalise_quantise_and_noise_are_the_reference_transforms(gold):
    fx = gold.npz("fx_f0norm.npz")
    for a, b in (("in_1xT", "out_1xT"), ("in_2xT", "out_2xT"), ("in_zero_row", "out_zero_row")):
        want, bar = _bar(lambda x: ref64.f0_normalise(x)[0], torch.from_numpy(fx[a]))
        err = float((want - torch.from_numpy(fx[b]).double()).abs().max())
        print(f"f0 normalise {a}: |ref64 - reference| = {err:.3e}, bar = {bar:.3e}")
        assert err <= bar, (a, err, bar)            # measured: err 3.1e-7 .. 4.2e-7 against bars 7.8e-7 .. 8.3e-7
        assert torch.equal(want == 0, torch.from_numpy(fx[a]) == 0)          # zeros stay zero, nothing else becomes zero
    want, bar = _bar(lambda x: ref64.f0_normalise(x)[0], torch.from_numpy(fx["in_2xT"]).unsqueeze(0))
    assert float((want - torch.from_numpy(fx["out_1x2xT"]).double()).abs().max()) <= bar
    # quantisation of the reference's own normalised track: x * 16, the rounding and / 16 are exact in both formats -> bar 0
    nf = torch.from_numpy(fx["out_2xT"]).unsqueeze(0).permute(1, 0, 2)
    want, bar = _bar(ref64.f0_quantise, nf, 16)
    assert bar == 0.0 and torch.equal(want, torch.from_numpy(fx["quant16"]).double())
    assert torch.equal(want.float(), of0.quantize(nf, 16))
    # additive noise, the reference's draw (seed 1234): one float32 addition
    from satools_amd import f0_transforms
    torch.manual_seed(1234)
    noise = f0_transforms.draw_awgn(nf.shape, f0_transforms.parse_awgn_db("quant_16_awgn_2"))
    wantn, bar = _bar(ref64.f0_awgn, want.float(), noise)
    err = float((wantn - torch.from_numpy(fx["quant16_awgn2_seed1234"]).double()).abs().max())
    print(f"f0 awgn: |ref64 - reference| = {err:.3e}, bar = {bar:.3e}")
    assert err <= bar, (err, bar)                   # measured: err 1.2e-7 against bar 2.4e-7 (the one addition)
    assert torch.equal(wantn == 0, want == 0)
    # half to even, not half away from zero
    ties = (torch.arange(-8, 8, dtype=torch.float32) + 0.5) / 16
    assert torch.equal(ref64.f0_quantise(ties, 16), torch.round(ties.double() * 16) / 16)
    assert float(ref64.f0_quantise(torch.tensor([2.5 / 16]), 16)) == 2.0 / 16


def test_mean_reversion_is_the_reference_and_the_oracle(gold):
    fx = gold.npz("fx_meanrev.npz")
    for T in ("T52", "T250"):
        x = torch.from_numpy(fx["in_" + T])
        for spec in ("mean-reverv_0.5:32", "mean-reverv_0.3:7", "mean-reverv_1:4"):
            alpha, n = of0.parse_mean_reverv(spec)
            want, bar = _bar(lambda v: ref64.mean_reversion(v, alpha, n)[0], x)
            err = float((want - torch.from_numpy(fx[f"{T}/{spec}"]).double()).abs().max())
            print(f"mean reversion {T} {spec}: |ref64 - reference| = {err:.3e}, bar = {bar:.3e}")
            assert want.shape == x.shape
            assert err <= bar, (T, spec, err, bar)      # measured: err 5.3e-8 .. 1.9e-7 against bars 1.1e-7 .. 3.0e-7
            assert float((want - of0.mean_reversion(x.clone(), alpha, n).double()).abs().max()) <= bar
    # windows longer than the track, a window of one, no blend / all average: against the oracle on random tracks
    g = torch.Generator().manual_seed(11)
    for T, n, alpha in ((1, 1, 0.5), (1, 32, 1.0), (5, 33, 0.5), (31, 2, 0.0), (33, 32, 0.5), (300, 33, 1.0)):
        x = torch.randn(1, 1, T, generator=g) * (torch.rand(1, 1, T, generator=g) > 0.3)
        want, bar = _bar(lambda v: ref64.mean_reversion(v, alpha, n)[0], x)
        err = float((want - of0.mean_reversion(x.clone(), alpha, n).double()).abs().max())
        print(f"mean reversion T={T} n={n} alpha={alpha}: |ref64 - oracle| = {err:.3e}, bar = {bar:.3e}")
        assert err <= bar, (T, n, alpha, err, bar)     # measured: err 0 .. 5.7e-8 against bars 0 .. 9.5e-8 (a bar of 0: exact on every side)


def test_attentive_stats_and_l2_norm_are_the_oracle_stages():
    sd = synthetic.xvector_state(0, 10)
    g = torch.Generator().manual_seed(12)
    C = sd["stat_pooling.linear1.weight"].shape[1]
    for B, T in ((1, 1), (2, 37), (1, 101)):
        h = torch.relu(torch.randn(B, C, T, generator=g))
        p = "stat_pooling."
        a = torch.tanh(F.conv1d(h, sd[p + "linear1.weight"], sd[p + "linear1.bias"]))
        logits = F.conv1d(a, sd[p + "linear2.weight"], sd[p + "linear2.bias"])          # the oracle's own logits, bit for bit
        ref = ox.attentive_stats_pool(sd, h).double()
        wm, bar_m = _bar(lambda x, l: ref64.attentive_stats(x, l)[0], h, logits)
        ws, bar_s = _bar(lambda x, l: ref64.attentive_stats(x, l)[1], h, logits)
        em, es = float((wm - ref[:, :C]).abs().max()), float((ws - ref[:, C:]).abs().max())
        print(f"attentive stats B={B} T={T}: mean err {em:.3e} (bar {bar_m:.3e}), std err {es:.3e} (bar {bar_s:.3e})")
        assert em <= bar_m, (B, T, em, bar_m)       # measured: err 0 .. 1.5e-7 against bars 0 .. 3.0e-7 (T = 1: the one weight is exactly 1)
        assert es <= bar_s, (B, T, es, bar_s)       # measured: err 1.7e-12 .. 1.7e-7 against bars 3.5e-12 .. 3.0e-7 (T = 1: every side clamps to sqrt(1e-9))
    for R, D in ((1, 192), (5, 192), (3, 7)):
        e = torch.randn(R, D, generator=g) * 3
        want, bar = _bar(lambda x: ref64.l2norm(x)[0], e)
        err = float((want - F.normalize(e, dim=1).double()).abs().max())
        print(f"l2 norm R={R} D={D}: err {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (R, D, err, bar)         # measured: err 8.7e-9 .. 5.9e-8 against bars 1.7e-8 .. 1.2e-7
    assert torch.equal(ref64.l2norm(torch.zeros(2, 5))[0], torch.zeros(2, 5, dtype=torch.float64))


def test_selections_are_torch_own():
    """nearest interpolation, replicate padding and the assembly are selections: float32 in, the same float32 out"""
    g = torch.Generator().manual_seed(13)
    x = torch.randn(3, 4, 5, generator=g)
    assert torch.equal(ref64.pad_replicate(x, 2, 3), F.pad(x, (2, 3), mode="replicate"))
    y = ref64.pad_replicate(x, 1, 4, interleave_right=True)
    assert y.shape == (3, 4, 10) and torch.equal(y[:, :, :6], F.pad(x, (1, 0), mode="replicate"))
    tiled = x[:, :, -1:].permute(2, 1, 0).repeat(1, 1, 4)               # pad_input: [1, C, B * right] -> cut into B pieces
    assert torch.equal(y[:, :, 6:], torch.stack(torch.split(tiled[0], 4, dim=1), 0))
    f0, spk = torch.randn(3, 7, generator=g), torch.randn(3, 2, generator=g)
    z = ref64.assemble_input(x, f0, spk)
    assert z.shape == (3, 4 + 1 + 2, 5) and torch.equal(z[:, :4], x) and torch.equal(z[:, 5:], spk.unsqueeze(2).expand(-1, -1, 5))
    assert torch.equal(z[:, 4], f0[:, [0, 1, 2, 4, 5]])                # floor(t * 7 / 5)
    ls, aux = ref64.log_softmax_channels(x * 60)
    assert float((ls - F.log_softmax((x * 60).double(), dim=1)).abs().max()) < 1e-12 and float(torch.exp(ls).sum(1).sub(1).abs().max()) < 1e-12
