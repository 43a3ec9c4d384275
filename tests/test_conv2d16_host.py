"""Host side of the split-f16 2-D convolutions (csrc/conv2d16/, include/satools_hip_conv2d16.h), CPU only: the weight packing, the
emulation of the kernel's arithmetic (tests/ref_split16.py) against float64 inside the bound of tests/test_hip_conv2d16.py and through the
whole ResNet against the reference's x-vectors, the header's constant and the conditions on that file's bounds rows (header, binding and
table are held together by tests/test_components_host.py), and the plumbing of `conv2d_precision`."""
import os
import re

import numpy as np
import pytest
import torch

import abi_decl
import ref_split16
import test_hip_conv2d16 as hc
from satools_amd import _lib, ops, packing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sat_conv2d_f16x3_f32"
HEADER = "satools_hip_conv2d16.h"


# ---- packing ---------------------------------------------------------------------------------------------------------------------
def _unpack(w_split, descale, cout, cin, k):
    """[Cin / 16, k k, 2, 2, Cout, 8] f16 -> (hi + lo) * descale as float64 [Cout, Cin, k, k]"""
    s = w_split.double().sum(2)                                                   # hi + lo: [chunk, tap, half, co, 8]
    return s.permute(3, 0, 2, 4, 1).reshape(cout, cin, k, k) * descale


@pytest.mark.parametrize("magnitude", [1e-5, 1.0, 1e4])
@pytest.mark.parametrize("cout,cin,k", [(32, 32, 3), (64, 32, 1), (128, 64, 3)])
def test_packing_carries_22_bits_at_every_magnitude(magnitude, cout, cin, k):
    g = torch.Generator().manual_seed(cout + cin + k)
    w = torch.randn(cout, cin, k, k, generator=g) * magnitude
    w[0, 0, 0, 0] = 0.0
    w_split, descale = ops.pack_conv2d_weight_f16x3(w)
    assert w_split.dtype == torch.float16 and tuple(w_split.shape) == (cin // 16, k * k, 2, 2, cout, 8) and w_split.is_contiguous()
    e = -int(round(np.log2(descale)))
    assert descale == 2.0 ** -e == w_split_scale(w)
    top = float(w_split[:, :, 0].double().abs().max())                            # the largest scaled magnitude (its hi half)
    assert 2.0 ** 9 <= float((w.double().abs().max() * 2.0 ** e)) < 2.0 ** 10 and 2.0 ** 9 <= top <= 2.0 ** 10
    err = (_unpack(w_split, descale, cout, cin, k) - w.double()).abs()
    bound = torch.maximum(2.0 ** -22 * w.double().abs(), torch.full_like(err, 2.0 ** -25 * 2.0 ** -e))
    assert bool((err <= bound).all()), float((err / bound).max())
    # the element order the header documents
    c, t, h, co, j = 1, k * k - 1, 1, 5, 3
    want = w[co, 16 * c + 8 * h + j, t // k, t % k].double() * 2.0 ** e
    assert abs(float(w_split[c, t, 0, h, co, j].double() + w_split[c, t, 1, h, co, j].double() - want)) <= 2.0 ** -22 * abs(float(want)) + 2.0 ** -25
    assert float(w_split[c, t, 0, h, co, j]) == float(want.float().half())


def w_split_scale(w):
    return 2.0 ** -packing.f16x3_scale_exponent(w)


def test_packing_transpose_zero_and_refusals():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(64, 32, 3, 3, generator=g)
    a, da = ops.pack_conv2d_weight_f16x3(w, transpose=True)
    b, db = ops.pack_conv2d_weight_f16x3(w.transpose(2, 3).contiguous())
    assert torch.equal(a, b) and da == db
    assert not torch.equal(a, ops.pack_conv2d_weight_f16x3(w)[0])
    z, dz = ops.pack_conv2d_weight_f16x3(torch.zeros(32, 32, 1, 1))
    assert dz == 1.0 and not bool(z.any())
    for bad in (float("nan"), float("inf"), -float("inf")):
        v = w.clone()
        v[3, 2, 1, 0] = bad
        with pytest.raises(packing.SplitRangeError):
            ops.pack_conv2d_weight_f16x3(v)
    for bad in (w.double(), w[:, :, :, :2], w[0], torch.randn(32, 8, 3, 3)):
        with pytest.raises(_lib.SatError):
            ops.pack_conv2d_weight_f16x3(bad)
    # the same split as the emulation's
    hi, lo, e = ref_split16.split_weight(w)
    assert 2.0 ** -e == ops.pack_conv2d_weight_f16x3(w)[1]
    assert torch.equal(_unpack(ops.pack_conv2d_weight_f16x3(w)[0], 1.0, 64, 32, 3), hi + lo)


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
def test_toward_zero_split_of_the_activations():
    v = torch.tensor([0.0, 1.0, -1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -10 + 2.0 ** -12, -(1.0 + 2.0 ** -11), 65519.0, -65519.99, 2.0 ** -14, 2.0 ** -15 + 2.0 ** -25,
                      -(2.0 ** -24 + 2.0 ** -26), 2.0 ** -25, 0.1, -3.3e-7])
    h = ref_split16.f16_toward_zero(v)
    assert h.tolist() == [0.0, 1.0, -1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -10, -1.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -15, -(2.0 ** -24), 0.0,
                          float(h[12]), float(h[13])]
    assert bool((h.abs() <= v.abs()).all()) and torch.equal(h.half().float(), h)  # toward zero, and f16 values
    near = v.half().float()                                                       # never farther than one f16 step from the nearest
    assert bool(((h - near).abs() <= torch.maximum(near.abs() * 2.0 ** -10, torch.tensor(2.0 ** -24))).all())
    hi, lo = ref_split16.split_activation(torch.randn(4096, generator=torch.Generator().manual_seed(2)) * 8)
    x = torch.randn(4096, generator=torch.Generator().manual_seed(2)) * 8
    assert bool(((hi + lo - x.double()).abs() <= torch.maximum(2.0 ** -20 * x.double().abs(), torch.tensor(2.0 ** -24, dtype=torch.float64))).all())


@pytest.mark.parametrize("cin,cout,stride,ksize", hc.NET_CONVS, ids=lambda v: str(v))
def test_emulation_stays_inside_the_gpu_tests_bound(cin, cout, stride, ksize):
    """the three products in float64 on the GPU test's inputs: what the split alone costs, before any GPU run"""
    worst = 0.0
    for key in hc.net_case_list(cin, cout, stride, ksize):
        c = hc.case(*key)
        r = hc.ratio(ref_split16.conv2d(c["x"], c["w"], stride, c["sc"], c["sh"], c["relu"]), c)
        worst = max(worst, r)
        assert r <= 1.0, (key, r)
    print(f"emulation {cin}->{cout} k{ksize} s{stride}: largest error / bound {worst:.4f}")


def test_emulation_stays_inside_the_bound_over_the_scale_sweep():
    for xs in hc.X_SCALES:
        for ws in hc.W_SCALES:
            c = hc.case(*hc.SWEEP, xs, ws)
            r = hc.ratio(ref_split16.conv2d(c["x"], c["w"], c["stride"], c["sc"], c["sh"], c["relu"]), c)
            print(f"emulation sweep x * {xs:g}, w * {ws:g}: error / bound {r:.4f}")
            assert r <= 1.0, (xs, ws, r)


@pytest.mark.parametrize("tag,seed,n", hc.UTTERANCES)
def test_emulated_resnet_meets_the_x_vector_bar(tag, seed, n):
    """the emulation carried through the whole ResNet: the x-vector against the reference's by the project's bar"""
    from satools_amd import synthetic
    from test_ref64_resnet import features64
    fx = np.load(os.path.join(hc.GOLD, "fx_xvector_resnet.npz"))
    sd = synthetic.xvector_resnet_state(0, 10)
    xv, _ = ref_split16.forward(sd, features64(sd, synthetic.harm_batch([seed], n)))
    got, ref = xv.numpy()[0], fx[tag + "/xvector"][0].astype(np.float64)
    err = float(np.abs(got - ref).max())
    cos = float((got * ref).sum() / (np.linalg.norm(got) * np.linalg.norm(ref)))
    print(f"{tag}: emulated split-f16 ResNet, x-vector max abs error vs reference {err:.2e}, cosine {cos:.9f}")
    assert err < 5e-6 and cos > 0.999999


# ---- what is particular to this component (tests/test_components_host.py holds header, binding, library, build and bounds table together) ----
def test_conv2d16_header_limit_is_the_largest_f16_and_the_emulations():
    text = abi_decl.define(HEADER, "SAT_CONV2D16_SPLIT_LIMIT")
    limit = float(re.fullmatch(r"([0-9.]+)f", text).group(1))
    assert limit == ref_split16.SPLIT_LIMIT == 65520.0
    assert float(torch.tensor(np.nextafter(np.float32(limit), np.float32(0))).half()) == 65504.0 and torch.isinf(torch.tensor(limit).half())
    assert len(_lib.COMPONENTS["conv2d16"][ENTRY][1]) == 16
    assert callable(ops.conv2d_f16x3) and callable(ops.pack_conv2d_weight_f16x3)


def test_the_conv2d16_bounds_rows_run_with_and_without_the_flag_and_the_epilogue():
    flags = {s[8] for r in hc.ROWS for s in r.shapes}
    epis = {s[7] for r in hc.ROWS for s in r.shapes}
    assert flags == {True, False} and {"none", "affine_relu"} <= epis


def test_the_gpu_tests_shapes_straddle_the_kernels_tiles():
    tile = open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "conv2d16_tile.h")).read()      # the tile body the kernel calls
    assert int(re.search(r"constexpr int C16_TH = (\d+);", tile).group(1)) == hc.TH == 4
    text = open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "conv2d16", "conv2d_f16x3.hip")).read()
    assert "SAT_C16(3, 1, 2, 2)" in text and "SAT_C16(3, 2, 1, 1)" in text       # 32 NT output columns: 64 at stride 1, 32 at stride 2
    assert {(3, 63), (4, 64), (5, 65)} <= set(hc.SHAPES)                          # below / at / above 4 x 64 at stride 1
    assert {(7, 63), (8, 64), (9, 65)} <= set(hc.SHAPES)                          # outputs 4x32, 4x32, 5x33 at stride 2: 2 TH - 1 .. and 2 TW2 - 1 ..
    assert [((h - 1) // 2 + 1, (w - 1) // 2 + 1) for h, w in ((7, 63), (8, 64), (9, 65))] == [(hc.TH, hc.TW2), (hc.TH, hc.TW2), (hc.TH + 1, hc.TW2 + 1)]


# ---- the net's plumbing ------------------------------------------------------------------------------------------------------------
def test_conv2d_precision_default_environment_and_cache_key(monkeypatch):
    from satools_amd import synthetic, xvector_resnet
    monkeypatch.delenv("SATOOLS_AMD_RESNET_CONV2D", raising=False)
    Net = xvector_resnet.build()
    assert Net.conv2d_precision == "f32" and Net.split_fallbacks == 0 and Net.last_conv2d_arithmetic is None
    monkeypatch.setenv("SATOOLS_AMD_RESNET_CONV2D", "f16x3")
    assert xvector_resnet.build().conv2d_precision == "f16x3"
    assert xvector_resnet.build().precision == Net.precision                      # the attention's precision is another attribute
    net = Net(num_speakers=10)
    net.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True)
    cpu = torch.device("cpu")
    W = net._prepare(cpu)
    key = net._cache_key
    assert not W["split2d"] and "w16" not in W["blocks"][0]["c1"]
    assert net._prepare(cpu) is W
    net.conv2d_precision = "f16x3"
    W16 = net._prepare(cpu)
    assert net._cache_key != key and W16 is not W and W16["split2d"]
    assert "w16" not in W16["stem"]                                                # the stem stays on the exact kernel
    n16 = 0
    for blk in W16["blocks"]:
        for name in ("c1", "c2", "sc"):
            e = blk[name]
            if e is not None:
                assert e["w16"].dtype == torch.float16 and e["w16"].shape[1] == e["k"] ** 2 and e["descale"] > 0 and "w" in e
                n16 += 1
    assert n16 == 36
    net.conv2d_precision = "f64"
    with pytest.raises(_lib.SatError, match="conv2d_precision"):
        net._prepare(cpu)


def test_asv_eval_option_reaches_the_attribute(monkeypatch, tmp_path, capsys):
    from satools_amd import asv_eval, infer_helper

    class Model:
        def to(self, device):
            return self

    class ResNetModel(Model):
        conv2d_precision = "f32"

    seen = {}
    monkeypatch.setattr(asv_eval, "test_metrics", lambda model, *a, **k: seen.setdefault("models", []).append(model) or {"eer": 0.0})
    args = ["ck", "--enrolls-wav-scp", "e", "--trails-wav-scp", "t", "--enroll-utt2spk", "u", "--trials", "l", "--decode-output", str(tmp_path)]
    monkeypatch.setattr(infer_helper, "load_model", lambda path: ResNetModel())
    asv_eval.main(args)
    assert "conv2d_precision" not in vars(seen["models"][-1])                     # without the option nothing is set
    asv_eval.main(args + ["--resnet-conv2d", "f16x3"])
    assert seen["models"][-1].conv2d_precision == "f16x3"
    asv_eval.main(args + ["--resnet-conv2d", "f32"])
    assert vars(seen["models"][-1])["conv2d_precision"] == "f32"
    monkeypatch.setattr(infer_helper, "load_model", lambda path: Model())          # the ECAPA model has no such attribute
    with pytest.raises(SystemExit):
        asv_eval.main(args + ["--resnet-conv2d", "f16x3"])
    with pytest.raises(SystemExit):
        asv_eval.main(args + ["--resnet-conv2d", "bf16"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        asv_eval.main(["--help"])
    assert "--resnet-conv2d {f32,f16x3}" in capsys.readouterr().out


def test_ops_conv2d_f16x3_checks_its_arguments_before_any_device_call(monkeypatch):
    def no_device_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "lib", no_device_call)
    w16, d = ops.pack_conv2d_weight_f16x3(torch.randn(64, 32, 3, 3))
    x = torch.zeros(1, 32, 4, 4)
    flag = torch.zeros(1, dtype=torch.int32)
    cases = {
        "x of three axes": lambda: ops.conv2d_f16x3(x[0], w16, d, 3),
        "x in float64": lambda: ops.conv2d_f16x3(x.double(), w16, d, 3),
        "f32 packing": lambda: ops.conv2d_f16x3(x, ops.pack_conv2d_weight(torch.randn(64, 32, 3, 3)), d, 3),
        "split weights in float32": lambda: ops.conv2d_f16x3(x, w16.float(), d, 3),
        "weights that are not contiguous": lambda: ops.conv2d_f16x3(x, w16.transpose(0, 1), d, 3),
        "weights of another Cin": lambda: ops.conv2d_f16x3(torch.zeros(1, 64, 4, 4), w16, d, 3),
        "weights of another ksize": lambda: ops.conv2d_f16x3(x, w16, d, 1),
        "scale of another length": lambda: ops.conv2d_f16x3(x, w16, d, 3, ch_scale=torch.zeros(32), ch_shift=torch.zeros(32)),
        "scale in float64": lambda: ops.conv2d_f16x3(x, w16, d, 3, ch_scale=torch.zeros(64).double(), ch_shift=torch.zeros(64)),
        "stride 0": lambda: ops.conv2d_f16x3(x, w16, d, 3, stride=0),
        "descale 0": lambda: ops.conv2d_f16x3(x, w16, 0.0, 3),
        "descale NaN": lambda: ops.conv2d_f16x3(x, w16, float("nan"), 3),
        "a flag of two elements": lambda: ops.conv2d_f16x3(x, w16, d, 3, overflow=torch.zeros(2, dtype=torch.int32)),
        "a flag in int64": lambda: ops.conv2d_f16x3(x, w16, d, 3, overflow=flag.long()),
    }
    for what, fn in cases.items():
        with pytest.raises(_lib.SatError):
            fn()
            pytest.fail(what)
    monkeypatch.undo()
    if not torch.cuda.is_available():                                             # no device: refused like every other op, no CPU fallback
        with pytest.raises(_lib.SatError, match="no CPU fallback"):
            ops.conv2d_f16x3(x, w16, d, 3, overflow=flag)
