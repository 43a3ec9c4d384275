"""tests/ref64_resnet.py restates the reference (CPU only): its whole forward in float64, from the waveform through ref64's front end,
against the outputs of the reference's own Net recorded in tests/golden/fx_xvector_resnet.npz.

BAR: the fixture is the reference's FLOAT32 forward, the restatement is float64.  The fixture records, per tensor, how far that float32
forward is from the same Net's own forward in float64 (`<name>_f32_dev`, the largest deviation over the tensor).  If the restatement
says what the reference says, it differs from the reference's float64 forward by float64 roundings only, hence from the fixture by
`_f32_dev`; the bar is twice that."""
import os

import numpy as np
import pytest
import torch

import ref64
import ref64_resnet

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UTTERANCES = (("harm0_16000", 0, 16000), ("harm3_48000", 3, 48000), ("harm7_24123", 7, 24123))
SUB = (4, 3, 3)          # tests/golden/make_xvector_resnet_fixtures.py


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "fx_xvector_resnet.npz"))


@pytest.fixture(scope="module")
def sd():
    from satools_amd import synthetic
    return synthetic.xvector_resnet_state(0, 10)


def features64(sd, wav):
    fb = sd["preprocessor.MelSpec.mel_scale.fb"].t()
    return ref64.instance_norm(ref64.logmel(wav, sd["preprocessor.MelSpec.spectrogram.window"], fb))[0]


@pytest.mark.parametrize("tag,seed,n", UTTERANCES)
def test_whole_forward_matches_the_reference(fx, sd, tag, seed, n):
    from satools_amd import synthetic
    xv, taps = ref64_resnet.forward(sd, features64(sd, synthetic.harm_batch([seed], n)))
    taps["xvector"] = xv
    for name in ("xvector", "pooled", "bn1", "layer1", "layer2", "layer3", "layer4"):
        got = taps[name]
        if got.dim() == 4:
            got = got[:, ::SUB[0], ::SUB[1], ::SUB[2]]
        want = torch.from_numpy(fx[f"{tag}/{name}"]).double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err, dev = float((got - want).abs().max()), float(fx[f"{tag}/{name}_f32_dev"])
        print(f"{tag} {name}: max |ref64 - fixture| {err:.3e}, recorded f32 deviation {dev:.3e}, ratio {err / dev:.3f}")
        assert err <= 2 * dev, (name, err, dev)


def test_fixture_covers_odd_and_even_sizes_under_stride_two(fx):
    frames = [1 + n // 160 for _, _, n in UTTERANCES]
    assert frames == [101, 301, 151]
    from satools_amd import xvector_resnet
    assert [xvector_resnet.pooled_frames(f) for f in frames] == [13, 38, 19]
    # widths the three stride-2 layers read: 101 / 301 / 151 (odd), 51 / 151 / 76 (both), 26 / 76 / 38 (even); the frequency axis is
    # 80 / 40 / 20, always even.  (Odd AND even at each single layer is what the kernel tests of tests/test_hip_xvector_resnet.py cover)
    sizes = [[f, (f - 1) // 2 + 1, ((f - 1) // 2) // 2 + 1] for f in frames]
    assert sizes == [[101, 51, 26], [301, 151, 76], [151, 76, 38]]
    assert {s[1] % 2 for s in sizes} == {0, 1}
    assert os.path.getsize(os.path.join(GOLD, "fx_xvector_resnet.npz")) < 1_000_000


def test_pieces_agree_with_torch_modules():
    """the restated pieces against torch's own modules in float64 (random data): conv + BatchNorm + ReLU, the SE block tail, the
    pooling with global context"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 8, 7, 9, generator=g)
    conv = torch.nn.Conv2d(8, 16, 3, stride=2, padding=1, bias=False).double()
    bn = torch.nn.BatchNorm2d(16).double().eval()
    with torch.no_grad():
        bn.running_mean.normal_(generator=g), bn.running_var.uniform_(0.5, 1.5, generator=g), bn.weight.uniform_(0.5, 1.5, generator=g), bn.bias.normal_(generator=g)
        want = torch.relu(bn(conv(x.double())))
        sc, sh = ref64_resnet.batchnorm_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var)
        got, aux = ref64_resnet.conv2d(x, conv.weight, 2, sc, sh, relu=True)
        assert float((got - want).abs().max()) < 1e-13 and bool((aux["S"] >= aux["sum"].abs() - 1e-12).all())
        xs = torch.randn(3, 20, 11, generator=g)
        mean, std, _ = ref64_resnet.mean_std(xs)
        assert float((mean - xs.double().mean(2)).abs().max()) < 1e-14 and float((std - xs.double().std(2)).abs().max()) < 1e-14
        assert bool(torch.isnan(ref64_resnet.mean_std(xs[:, :, :1])[1]).all())
        att = torch.nn.Sequential(torch.nn.Conv1d(60, 6, 1), torch.nn.ReLU(), torch.nn.BatchNorm1d(6), torch.nn.Tanh(), torch.nn.Conv1d(6, 20, 1),
                                  torch.nn.Softmax(dim=2)).double().eval()
        att[2].running_mean.normal_(generator=g), att[2].running_var.uniform_(0.5, 1.5, generator=g)
        xd = xs.double()
        w = att(torch.cat([xd, torch.cat([xd.mean(2), xd.std(2)], 1).unsqueeze(2).repeat(1, 1, 11)], dim=1))
        mu = (xd * w).sum(2)
        want = torch.cat([mu, torch.sqrt(((xd ** 2 * w).sum(2) - mu ** 2).clamp(min=1e-9))], 1)
        sc, sh = ref64_resnet.batchnorm_affine(att[2].weight, att[2].bias, att[2].running_mean, att[2].running_var)
        got = ref64_resnet.attentive_pooling_gc(xs, att[0].weight, att[0].bias, sc, sh, att[4].weight, att[4].bias)[0]
        assert float((got - want).abs().max()) < 1e-12
    z, r, gl = torch.randn(2, 4, 3, 5, generator=g), torch.randn(2, 4, 3, 5, generator=g), torch.randn(2, 4, generator=g)
    y, aux = ref64_resnet.se_scale_add_relu(z, gl, r)
    assert float((y - torch.relu(z.double() * torch.sigmoid(gl.double())[:, :, None, None] + r.double())).abs().max()) < 1e-15
