"""ResNet x-vector extractor (egs/asv/voxceleb/local/tuning/resnet.py) on the HIP device.  Needs a real MI355X: run with `-m gpu`.

Two kinds of test.
(1) Every new kernel against the float64 restatements of tests/ref64_resnet.py with DERIVED bounds (U = 2^-24 from ref64; a wave sum
    of n terms collects ref64.reduction_terms(n) roundings):
      sat_conv2d_f32             |err| <= (9 Cin + 4) U sum|w x| |scale|  +  U |sum scale|  +  U |sum scale + shift|
                                 (any summation order of K <= 9 Cin products; one rounding for the scale, one for the shift; the ReLU is
                                 exact on its input)
      sat_se_scale_add_relu_f32  gate = 1 / (1 + expf(-g)): (EXP_ULP ULP + 2 U) relative; the product U, the add U of its result
      sat_row_mean_std_f32       mean: k(T) U sum|x| / T.  Deviation: every d = x - mean carries the mean's error and its own rounding;
                                 sum d^2 collects k(T) roundings; the divide and the root one each (interval form, right at S2 = 0)
      the pooling composition    Net.pool's intermediate tensors: the hidden layer (frames' 2560-term product, the context's 5120-term
                                 matrix-vector product, ReLU, BatchNorm affine, tanh), the logits, and the pooled statistics by
                                 test_hip_small_kernels' bound for attentive_stats widened by the logits' own error (a shift of all
                                 logits of a row by at most eps changes every softmax weight by at most e^(2 eps) - 1 relative).
                                 Per product of the two 1x1 convs: U in "f32" precision; 2^-21 in "f16x3" plus the split's documented
                                 absolute floor 2^-24 sum|w| (split-f16 range).
    The largest error / bound per kernel is printed and, if SAT_XVECTOR_RESNET_RATIOS names a file, written there
    (profiles/xvector_resnet_error_ratios.txt).  A ratio above 1 is a bug.
(2) The net against the reference's own outputs (tests/golden/fx_xvector_resnet.npz): the x-vector by the project's bar for that
    quantity (max abs error < 5e-6, cosine > 0.999999, | ||x|| - 1 | < 1e-5: test_hip_xvector.py), the intermediate tensors within
    8 x the recorded float32-vs-float64 deviation of the reference itself; batches, determinism, the checkpoint round trip, asv-eval.

MEASURED on an MI355X (profiles/xvector_resnet_error_ratios.txt), largest error / bound: conv2d 0.017 (MFMA kernel, every shape), 0.45 (stem) |
se_scale_add_relu 0.96 | row_mean_std 0.26 / 0.26 | pooling: context 0.31, hidden 0.0007, logits and mean < 0.0001, deviation 0.92 (B = 1, T' = 2) |
x-vector 1.4-1.8e-7 from the reference (bar 5e-6), cosine 1.0000000 | intermediates 0.19-1.38 x the reference's own f32 deviation (bar 8 x) |
test_metrics scores 0.06.  The file's 64 tests take 4.4 s on the GPU."""
import json
import os

import numpy as np
import pytest
import torch

import ref64
import ref64_asv
import ref64_resnet
from ref64 import U, reduction_terms

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ULP = 2.0 * U
EXP_ULP, TANH_ULP = 1, 2        # HIP math API: maximum ULP error of expf / tanhf
TINY = 2.0 ** -126
TH, TW = 4, 32                  # csrc/conv2d.hip: output rows / columns per block
UTTERANCES = (("harm0_16000", 0, 16000), ("harm3_48000", 3, 48000), ("harm7_24123", 7, 24123))
SUB = (4, 3, 3)                 # tests/golden/make_xvector_resnet_fixtures.py

# every (Cin, Cout, stride, ksize) of the net: the stem, layer1 (with its 1x1 stride-1 shortcut), then per later layer the stride-2
# 3x3, the 3x3 that follows, the 1x1 stride-2 shortcut
NET_CONVS = ((1, 32, 1, 3), (32, 32, 1, 3), (32, 32, 1, 1), (32, 64, 2, 3), (64, 64, 1, 3), (32, 64, 2, 1), (64, 128, 2, 3),
             (128, 128, 1, 3), (64, 128, 2, 1), (128, 256, 2, 3), (256, 256, 1, 3), (128, 256, 2, 1))
# H x W: 1, 2, 3; one below / at / one above the tile (4 rows, 32 columns; under stride 2 the INPUT sizes 7 / 8 / 9 and 63 / 64 / 65 give
# those output sizes); odd and even under stride 2
SHAPES = ((1, 1), (2, 3), (3, 2), (3, 31), (4, 32), (5, 33), (7, 63), (8, 64), (9, 65), (2, 66))
EPILOGUES = ("none", "affine", "affine_relu", "relu")

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    lines = [f"{k:34s} {r:8.4f}   at {case}" for k, (r, case) in sorted(_RATIOS.items())]
    print("\nlargest observed error / derived bound (kernels) or error / bar (net), per quantity:\n" + "\n".join(lines))
    path = os.environ.get("SAT_XVECTOR_RESNET_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_xvector_resnet.py: largest observed error / bound, per quantity (a ratio above 1 fails)\n")
            f.write("\n".join(lines) + "\n")


def _ops():
    import satools_amd  # noqa: F401
    from satools_amd import ops
    return ops


def _sat_error():
    from satools_amd import _lib
    return _lib.SatError


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _note(name, r, case):
    if r > _RATIOS.get(name, (-1.0, ""))[0]:
        _RATIOS[name] = (r, case)


def _check(kernel, case, got, want, bound, quiet=True):
    got = torch.as_tensor(got).detach().cpu().double()
    want, bound = torch.as_tensor(want).double(), torch.as_tensor(bound, dtype=torch.float64)
    assert got.shape == want.shape, (kernel, case, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), (kernel, case, "non-finite output")
    err = (got - want).abs()
    bound = bound.expand_as(err)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = float(ratio.max()) if ratio.numel() else 0.0
    if not quiet:
        print(f"{kernel} [{case}]: max error {float(err.max()):.3e}, max error / bound {r:.4f}")
    _note(kernel, r, case)
    assert r <= 1.0, (kernel, case, r, float(err.max()))
    return r


# ---- sat_conv2d_f32 ----------------------------------------------------------------------------------------------------------
def _conv_case(cin, cout, stride, ksize, B, H, W, epi):
    ops = _ops()
    g = _gen(1, cin, cout, stride, ksize, B, H, W, len(epi))
    x = torch.randn(B, cin, H, W, generator=g)
    if B > 1:
        x[1] *= -0.5
    w = torch.randn(cout, cin, ksize, ksize, generator=g) * (cin * ksize * ksize) ** -0.5       # asymmetric in every axis
    sc = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.2, -1.0, 1.0) if "affine" in epi else None
    sh = torch.randn(cout, generator=g) if "affine" in epi else None
    relu = "relu" in epi
    want, a = ref64_resnet.conv2d(x, w, stride, sc, sh, relu)
    k = 9 * cin + 4
    if sc is None:
        bound = k * U * a["S"]
    else:
        s64 = sc.double().view(1, -1, 1, 1)
        bound = k * U * a["S"] * s64.abs() + U * (a["sum"] * s64).abs() + U * a["affine"].abs()
    dev = lambda t: None if t is None else t.to(DEV)
    got = ops.conv2d(x.to(DEV), ops.pack_conv2d_weight(w.to(DEV)), ksize, stride, ch_scale=dev(sc), ch_shift=dev(sh), relu=relu)
    assert got.shape == (B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1)
    _check(f"conv2d k{ksize} s{stride}" + (" stem" if cin == 1 else ""), f"{cin}->{cout} B{B} {H}x{W} {epi}", got, want, bound)
    return got


@pytest.mark.parametrize("cin,cout,stride,ksize", NET_CONVS, ids=lambda v: str(v))
def test_conv2d_against_float64(cin, cout, stride, ksize):
    for i, (H, W) in enumerate(SHAPES):
        _conv_case(cin, cout, stride, ksize, 1, H, W, EPILOGUES[i % 4])
    for epi in EPILOGUES:                                                       # every epilogue option on one shape, and the batch
        _conv_case(cin, cout, stride, ksize, 1, 5, 33, epi)
    _conv_case(cin, cout, stride, ksize, 33, 6, 35, "affine_relu")
    _conv_case(cin, cout, stride, ksize, 33, 3, 2, "none")


def test_conv2d_transposed_weights_commute_with_transposed_images():
    """what the net relies on to keep time innermost: conv(x^T, w^T) = conv(x, w)^T.  The same products per output, summed with the
    taps in the other order: both within the conv's bound of the float64 value"""
    ops = _ops()
    g = _gen(2)
    x, w = torch.randn(2, 64, 9, 37, generator=g), torch.randn(128, 64, 3, 3, generator=g) / 24
    a = ops.conv2d(x.to(DEV), ops.pack_conv2d_weight(w.to(DEV)), 3, 2)
    b = ops.conv2d(x.transpose(2, 3).contiguous().to(DEV), ops.pack_conv2d_weight(w.to(DEV), transpose=True), 3, 2)
    want, aux = ref64_resnet.conv2d(x, w, 2)
    bound = (9 * 64 + 4) * U * aux["S"]
    _check("conv2d transposed", "64->128 9x37 s2", b.transpose(2, 3), want, bound)
    _check("conv2d transposed", "64->128 9x37 s2 (plain)", a, want, bound)


def test_conv2d_is_deterministic_and_refuses_other_shapes():
    ops, SatError = _ops(), _sat_error()
    g = _gen(3)
    x, w = torch.randn(3, 128, 10, 63, generator=g).to(DEV), ops.pack_conv2d_weight(torch.randn(128, 128, 3, 3, generator=g).to(DEV))
    assert torch.equal(ops.conv2d(x, w, 3), ops.conv2d(x, w, 3))
    z = lambda *s: torch.zeros(*s, device=DEV)
    for bad in (lambda: ops.conv2d(z(1, 48, 4, 4), z(9, 48, 64), 3),                  # Cin outside {32, 64, 128, 256}
                lambda: ops.conv2d(z(1, 32, 4, 4), z(9, 32, 96), 3),                  # Cout
                lambda: ops.conv2d(z(1, 32, 4, 4), z(25, 32, 32), 5),                 # 5x5
                lambda: ops.conv2d(z(1, 32, 4, 4), z(9, 32, 32), 3, stride=3),
                lambda: ops.conv2d(z(1, 1, 4, 4), z(9, 1, 64), 3),                    # Cin = 1 is the stem only
                lambda: ops.conv2d(z(1, 1, 4, 4), z(9, 1, 32), 3, stride=2),
                lambda: ops.conv2d(z(1, 32, 4, 4), z(9, 32, 32), 3, ch_scale=z(32)),   # scale without shift
                lambda: ops.conv2d(z(1, 32, 4, 4), z(9, 64, 32), 3)):                 # weights of another Cin
        with pytest.raises(SatError):
            bad()
    y = ops.conv2d(torch.ones(1, 1, 2, 2, device=DEV), torch.ones(9, 1, 32, device=DEV), 3)      # no sticky error: a valid call is right
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.full((1, 32, 2, 2), 4.0))


# ---- sat_se_scale_add_relu_f32 -----------------------------------------------------------------------------------------------
GATE_LOGITS = (-100.0, -20.0, 0.0, 20.0, 100.0)


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 1, 1), (2, 5, 7, 9), (1, 7, 8, 32), (2, 5, 5, 51), (33, 5, 3, 43), (1, 32, 80, 101), (1, 3, 1, 4099)], ids=lambda v: str(v))
def test_se_scale_add_relu(B, C, H, W):
    ops = _ops()
    g = _gen(4, B, C, H, W)
    z, r = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    logits = torch.tensor([GATE_LOGITS[(b + c) % 5] for b in range(B) for c in range(C)]).view(B, C)
    logits = torch.where(torch.rand(B, C, generator=g) < 0.5, torch.randn(B, C, generator=g) * 3, logits)
    want, a = ref64_resnet.se_scale_add_relu(z, logits, r)
    bound = a["prod"] * (EXP_ULP * ULP + 2 * U + U) + U * a["pre"].abs() + TINY * z.double().abs()
    got = ops.se_scale_add_relu(z.to(DEV), logits.to(DEV), r.to(DEV))
    _check("se_scale_add_relu", f"B{B}-C{C}-{H}x{W}", got, want, bound)
    assert float(got.min()) >= 0.0


def test_se_scale_add_relu_refuses_mismatched_shapes():
    z = torch.zeros(2, 4, 3, 5, device=DEV)
    with pytest.raises(_sat_error()):
        _ops().se_scale_add_relu(z, torch.zeros(2, 4, device=DEV), z[:, :, :, :-1])


# ---- sat_row_mean_std_f32 ----------------------------------------------------------------------------------------------------
def _mean_std_bounds(x, mean, std, a):
    T = x.shape[-1]
    k = reduction_terms(T)
    dm = k * U * a["S1"] / T
    dmax = (x.double() - mean.unsqueeze(-1)).abs().max(-1).values
    e = dm + U * (dmax + dm)                                                     # error of one d = x - mean
    dq = 2 * e * torch.sqrt(T * a["S2"]) + T * e * e + (k + 1) * U * (a["S2"] + 2 * e * torch.sqrt(T * a["S2"]) + T * e * e)
    lo, hi = torch.sqrt((a["S2"] - dq).clamp(min=0) / (T - 1)), torch.sqrt((a["S2"] + dq) / (T - 1))
    return dm, torch.maximum(std - lo, hi - std) + 2 * U * hi


@pytest.mark.parametrize("kind", ("randn", "mean100_std0.01", "constant"))
@pytest.mark.parametrize("B,C,T", [(1, 1, 2), (2, 5, 3), (1, 4, 13), (2, 3, 38), (1, 5, 63), (33, 2, 64), (2, 3, 65), (1, 2560, 19), (2, 3, 1000)], ids=lambda v: str(v))
def test_row_mean_std(kind, B, C, T):
    ops = _ops()
    g = _gen(5, B, C, T, len(kind))
    x = torch.randn(B, C, T, generator=g)
    if kind == "mean100_std0.01":
        x = (100.0 + 0.01 * x).float()
    elif kind == "constant":
        x = (torch.randn(B, C, 1, generator=g) * 10).expand(B, C, T).contiguous()
    mean, std, a = ref64_resnet.mean_std(x)
    dm, ds = _mean_std_bounds(x, mean, std, a)
    out = ops.row_mean_std(x.to(DEV)).cpu()
    assert out.shape == (B, 2 * C)
    _check("row_mean_std.mean", f"{kind}-B{B}-C{C}-T{T}", out[:, :C], mean, dm)
    _check("row_mean_std.std", f"{kind}-B{B}-C{C}-T{T}", out[:, C:], std, ds)


def test_row_mean_std_refuses_one_frame():
    with pytest.raises(_sat_error(), match="T >= 2"):
        _ops().row_mean_std(torch.zeros(1, 4, 1, device=DEV))


# ---- the net -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    import satools_amd  # noqa: F401
    from satools_amd import synthetic, xvector_resnet
    m = xvector_resnet.build()(num_speakers=10)
    m.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "fx_xvector_resnet.npz"))


@pytest.mark.parametrize("precision", ("f32", "f16x3"))
@pytest.mark.parametrize("B,T", [(1, 2), (2, 13), (1, 38), (2, 63)], ids=lambda v: str(v))
def test_pooling_composition_against_float64(net, precision, B, T):
    """Net.pool (global context as a per-utterance bias of the first 1x1 conv) against AttentivePooling.forward restated with the
    concatenated 7680-channel input, stage by stage"""
    from test_hip_small_kernels import _attentive_bounds
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    p = "stat_pooling.attention."
    g = _gen(6, B, T)
    x = torch.relu(torch.randn(B, 2560, T, generator=g) * 3)                    # what the last block's ReLU hands over
    sc, sh = ref64_resnet.batchnorm_affine(sd[p + "2.weight"], sd[p + "2.bias"], sd[p + "2.running_mean"], sd[p + "2.running_var"])
    want, aux = ref64_resnet.attentive_pooling_gc(x, sd[p + "0.weight"], sd[p + "0.bias"], sc, sh, sd[p + "4.weight"], sd[p + "4.bias"])
    try:
        net.precision = precision                                              # an instance attribute over the class's default
        taps = {}
        got = net.pool(x.to(DEV), taps)
    finally:
        del net.precision
    assert got.shape == (B, 5120, 1)
    up = U if precision == "f32" else 2.0 ** -21                                # per product of the 1x1 convs
    floor = 0.0 if precision == "f32" else 2.0 ** -24                           # f16x3: absolute floor per input element, times sum |w|
    w0, w4 = sd[p + "0.weight"].double()[:, :, 0], sd[p + "4.weight"].double()[:, :, 0]
    # global context
    mean, std, a_ms = ref64_resnet.mean_std(x)
    dm, ds = _mean_std_bounds(x, mean, std, a_ms)
    _check("pool.context", f"{precision}-B{B}-T{T}", taps["gc"], torch.cat([mean, std], 1), torch.cat([dm, ds], 1))
    # hidden layer: frames' product (2560 terms at `up`), the context's (5120 terms on one wave, the inputs' own error dgc), their sum,
    # the ReLU (exact), scale and shift (U each), tanh (TANH_ULP; 1-Lipschitz)
    gc_abs = torch.cat([mean, std], 1).abs()
    S_fr = torch.einsum("ak,bkt->bat", w0[:, :2560].abs(), x.double().abs())
    S_ctx = (gc_abs @ w0[:, 2560:].abs().t() + sd[p + "0.bias"].double().abs()).unsqueeze(2)
    d_ctx = (torch.cat([dm, ds], 1) @ w0[:, 2560:].abs().t()).unsqueeze(2) + (reduction_terms(5120) + 1) * U * S_ctx
    d_lin = (2560 + 4) * up * S_fr + floor * w0[:, :2560].abs().sum(1).view(1, -1, 1) + d_ctx + U * aux["lin"].abs()
    pre = torch.relu(aux["lin"]) * sc.view(1, -1, 1) + sh.view(1, -1, 1)
    d_a = d_lin * sc.abs().view(1, -1, 1) + U * (pre - sh.view(1, -1, 1)).abs() + U * pre.abs() + TANH_ULP * ULP * aux["a"].abs() + 2.0 ** -149
    _check("pool.hidden", f"{precision}-B{B}-T{T}", taps["a"], aux["a"], d_a)
    # logits: 128 terms at `up` on the computed hidden layer, whose own error enters through |w4|
    d_log = (128 + 4) * up * aux["S_logits"] + floor * w4.abs().sum(1).view(1, -1, 1) + torch.einsum("da,bat->bdt", w4.abs(), d_a) + U * aux["logits"].abs()
    _check("pool.logits", f"{precision}-B{B}-T{T}", taps["logits"], aux["logits"], d_log)
    # pooled statistics: attentive_stats' own bound, every weight further off by e^(2 eps) - 1, eps = the row's largest logit error
    eps = d_log.max(-1).values
    wrel = torch.expm1(2 * eps)
    mean_w, std_w = want[:, :2560], want[:, 2560:]
    dm1, dstd = _attentive_bounds(dict(aux), mean_w, std_w, T)
    dm1 = dm1 + wrel * aux["S1"]
    dvar = wrel * aux["S2"] + 2 * mean_w.abs() * wrel * aux["S1"] + (wrel * aux["S1"]) ** 2
    c = ref64.f32(1e-9)
    dstd = dstd + torch.maximum(std_w - torch.sqrt((aux["var"] - dvar).clamp(min=c)), torch.sqrt((aux["var"] + dvar).clamp(min=c)) - std_w)
    _check("pool.mean", f"{precision}-B{B}-T{T}", got[:, :2560, 0], mean_w, dm1)
    _check("pool.std", f"{precision}-B{B}-T{T}", got[:, 2560:, 0], std_w, dstd)


@pytest.mark.parametrize("tag,seed,n", UTTERANCES)
def test_xvector_and_intermediates_match_the_reference(net, fx, tag, seed, n):
    from satools_amd import synthetic
    wav = synthetic.harm_batch([seed], n)
    taps = {}
    (loss, logits), xv = net(wav[0].to(DEV), taps=taps)
    assert xv.shape == (1, 256) and torch.isnan(loss) and logits is None
    got = xv.cpu().numpy()
    ref = fx[tag + "/xvector"]
    cos = float((got.astype(np.float64) * ref).sum() / (np.linalg.norm(got.astype(np.float64)) * np.linalg.norm(ref.astype(np.float64))))
    err = float(np.abs(got - ref).max())
    print(f"{tag}: x-vector max abs error vs reference {err:.2e} (its own f32 deviation {float(fx[tag + '/xvector_f32_dev']):.2e}), cosine {cos:.8f}")
    _note("net x-vector error / 5e-6", err / 5e-6, tag)
    assert err < 5e-6 and cos > 0.999999
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-5
    for name in ("bn1", "layer1", "layer2", "layer3", "layer4", "pooled"):
        t = taps[name].cpu()
        if t.dim() == 4:
            t = t.transpose(2, 3)[:, ::SUB[0], ::SUB[1], ::SUB[2]]                # [B, C, F, T] here, [B, C, T, F] there
        else:
            t = t[:, :, 0]
        want = torch.from_numpy(fx[f"{tag}/{name}"])
        assert t.shape == want.shape, (name, t.shape, want.shape)
        dev = float(fx[f"{tag}/{name}_f32_dev"])
        e = float((t.double() - want.double()).abs().max())
        print(f"{tag} {name}: max abs error {e:.3e}, reference's own f32 deviation {dev:.3e}, ratio {e / dev:.3f} (bar 8)")
        _note(f"net {name} error / (8 f32_dev)", e / (8 * dev), tag)
        assert e <= 8 * dev, (name, e, dev)


def test_batch_determinism_and_checkpoint_round_trip(net, tmp_path):
    import satools_amd
    from satools_amd import synthetic
    wav = synthetic.harm_batch([1, 2], 16000).to(DEV)
    both = net(wav)[1]
    for i in range(2):
        assert torch.allclose(both[i], net(wav[i])[1][0], atol=1e-6)
    assert torch.equal(net(wav)[1], both)                                         # the same input gives the same bits
    ck = {"task_path": "/egs/asv/voxceleb", "base_model_path": "local/tuning/resnet.py", "base_model_params": {"num_speakers": 10},
          "base_model_args": {}, "base_model_state_dict": synthetic.xvector_resnet_state(0, 10)}
    torch.save(ck, tmp_path / "final.pt")
    m = satools_amd.load_model(str(tmp_path / "final.pt")).to(DEV)
    assert torch.equal(m(wav[0])[1], net(wav[0])[1])


def test_short_utterances_and_cpu_input_are_refused(net):
    SatError = _sat_error()
    with pytest.raises(SatError, match="pooled frame"):
        net(torch.zeros(1279, device=DEV))                                       # 8 frames -> one pooled frame
    assert net(torch.zeros(1, 1280, device=DEV) + 0.01)[1].shape == (1, 256)     # 9 frames -> two
    with pytest.raises(SatError):
        net(torch.zeros(16000))


def test_test_metrics_on_a_toy_directory(tmp_path):
    """asv_eval.test_metrics with the ResNet extractor, on the toy directory of tests/test_hip_asv_score.py"""
    import satools_amd
    from satools_amd import asv_eval, pipeline, synthetic
    model = satools_amd.load_model("synthetic:xvector_resnet?speakers=12").to(DEV)
    wavs = tmp_path / "wav"
    wavs.mkdir()
    enroll = {"spkA-u1": 0, "spkA-u2": 1, "spkB-u1": 2, "spkC-u1": 3, "spkC-u2": 4, "spkC-u3": 5}
    trial = {"spkA-u2": 1, "spkA-t1": 6, "spkB-t1": 7, "spkC-t1": 8, "spkB-t2": 9}         # spkA-u2 is in both lists
    for name, seed in {**enroll, **trial}.items():
        pipeline.save_pcm16(wavs / (name + ".wav"), synthetic.harm_utterance(seed, 16000 + 1601 * seed).unsqueeze(0), 16000)
    (tmp_path / "enroll.scp").write_text("".join(f"{n} {wavs / (n + '.wav')}\n" for n in enroll))
    (tmp_path / "trials.scp").write_text("".join(f"{n} {wavs / (n + '.wav')}\n" for n in trial))
    (tmp_path / "utt2spk").write_text("".join(f"{n} {n.split('-')[0]}\n" for n in enroll))
    tl = [(s, u, "target" if u.startswith(s) else "nontarget") for s in ("spkA", "spkB", "spkC") for u in trial]
    (tmp_path / "trials").write_text("".join(" ".join(t) + "\n" for t in tl))
    out = tmp_path / "out"
    m = asv_eval.test_metrics(model, str(tmp_path / "enroll.scp"), str(tmp_path / "trials.scp"), str(tmp_path / "utt2spk"),
                              str(tmp_path / "trials"), str(out))
    z = np.load(out / "xvectors.npz")
    xv = {str(u): torch.from_numpy(v) for u, v in zip(z["utts"], z["xvectors"])}
    assert set(xv) == set(enroll) | set(trial) and z["xvectors"].shape == (10, 256)
    spk2utt = {}
    for n in enroll:
        spk2utt.setdefault(n.split("-")[0], []).append(n)
    speakers = list(spk2utt)
    rows = [u for s in speakers for u in spk2utt[s]]
    offsets = np.concatenate([[0], np.cumsum([len(spk2utt[s]) for s in speakers])])
    X = torch.stack([xv[u] for u in rows])
    e64, eaux = ref64_asv.segment_mean_l2norm(X, np.arange(len(rows)), offsets)
    de = ref64_asv.segment_bound(e64, eaux, 256).norm(dim=1)                   # the enrolment vector's own error, as a 2-norm
    tn = list(trial)
    T = torch.stack([xv[u] for u in tn])
    ie = [speakers.index(s) for s, _, _ in tl]
    it = [tn.index(u) for _, u, _ in tl]
    s64, _, aux = ref64_asv.trial_scores(e64, T, ie, it)
    # a perturbation da of a unit vector a moves its cosine with anything by at most 2 |da|
    bound = ref64_asv.score_bound(s64, aux, 256) + 2 * de[torch.as_tensor(ie)]
    lines = [l.split() for l in open(out / "scores")]
    assert [(l[0], l[1]) for l in lines] == [(s, u) for s, u, _ in tl]
    _check("test_metrics scores (ResNet)", "toy directory", torch.tensor([float(l[2]) for l in lines], dtype=torch.float64), s64, bound)
    mj = json.load(open(out / "metric.json"))
    keys = {"linkability", "eer", "eer_lower", "eer_upper", "min_cllr", "eer_threshold"}
    assert set(mj) == keys | {"asnorm"} and set(mj["asnorm"]) == keys
    assert mj["asnorm"]["eer"] is not None and m["eer"] == mj["eer"]           # the cohort of 12 speakers was used (k = 12)
