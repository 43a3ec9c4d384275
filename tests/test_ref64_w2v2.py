"""tests/ref64_w2v2.py — the float64 references the wav2vec2 / fbank kernel tests (test_hip_w2v2_kernels.py) compare against — pinned on the
CPU against independent computations (torch.nn.functional in float64, the oracle's _SelfAttention, the oracle's fbank with pad_input), so
that they cannot drift; the stated accuracy of the fast GELUs checked on a grid; and the attention bound of the GPU test shown to tell a
right kernel from a wrong one on the GPU test's own cases.

Every bar of a pin is the error of float32 arithmetic against float64, measured here as test_ref64.py does: the same formula is evaluated
in float32 torch (ref64.in_float32()), and twice its largest deviation from the float64 result is the bar.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref64
import ref64_w2v2 as R
import test_hip_w2v2_kernels as K
from oracle import fbank as ofb
from oracle import tdnnf as otd
from oracle import wav2vec2 as ow2
from ref64 import U


def _bar(fn, *args):
    """(float64 result, 2 x max |float32 evaluation - float64 result|) of one ref64_w2v2 formula"""
    want = fn(*args)
    with ref64.in_float32():
        low = fn(*args)
    assert low.dtype == torch.float32 and want.dtype == torch.float64
    return want, 2.0 * float((low.double() - want).abs().max())


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---- pins ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,k,stride,n", [(512, 10, 5, 4005), (1, 1, 1, 7), (5, 3, 2, 24), (100, 16, 7, 1000), (1024, 15, 5, 93)])
def test_conv0_is_conv1d(Cn, k, stride, n):
    g = _g(Cn + k)
    x, w, b = torch.randn(3, n, generator=g) * 0.3, torch.randn(Cn, k, generator=g) * 0.3, torch.randn(Cn, generator=g) * 0.1
    want, bar = _bar(lambda *a: R.conv0(*a, stride)[0], x, w, b)
    ref = F.conv1d(x.double().unsqueeze(1), w.double().unsqueeze(1), b.double(), stride=stride)
    err = float((want - ref).abs().max())
    print(f"conv0 C={Cn} k={k} stride={stride}: |ref64 - F.conv1d| = {err:.3e}, bar = {bar:.3e}")
    assert want.shape == ref.shape and err <= bar          # measured: err 0 (the same products in the same order) against bars 2.1e-8 .. 6.5e-7
    S = R.conv0(x, w, b, stride)[1]["S"]
    assert bool((S >= want.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("Cn,T", [(1, 5), (5, 33), (100, 32), (513, 31), (1024, 65)])
@pytest.mark.parametrize("gelu,split", [(False, False), (True, True), (True, False), (False, True)])
def test_layernorm_channels_is_layer_norm(Cn, T, gelu, split):
    g = _g(Cn + T)
    x = torch.randn(2, Cn, T, generator=g) * 3 + 0.5
    gamma, beta = 1 + 0.5 * torch.randn(Cn, generator=g), 0.5 * torch.randn(Cn, generator=g)
    want, bar = _bar(lambda *a: R.layernorm_channels(*a, 1e-5, gelu, split)[0], x, gamma, beta)
    ref = F.layer_norm(x.double().permute(0, 2, 1), (Cn,), gamma.double(), beta.double(), ref64.f32(1e-5)).permute(0, 2, 1)
    if gelu:
        ref = F.gelu(ref)
    if split:
        ev, od = ref[:, :, 0::2], ref[:, :, 1::2]
        ref = torch.cat([ev, F.pad(od, (0, ev.shape[2] - od.shape[2]))], 1)
    err = float((want - ref).abs().max())
    print(f"layernorm C={Cn} T={T} gelu={gelu} split={split}: |ref64 - F.layer_norm| = {err:.3e}, bar = {bar:.3e}")
    assert want.shape == ref.shape and err <= bar          # measured: err <= 2.7e-15 against bars 6.5e-7 .. 2.3e-6 (C = 1: both sides give beta, bar 0; 8.1e-9 through the GELU)
    if split and T % 2:
        assert not want[:, Cn:, -1].any()


@pytest.mark.parametrize("G,T", [(1, 1), (3, 17), (2, 249)])
@pytest.mark.parametrize("scale", (0.125, 1.0))
def test_softmax_columns_is_softmax(G, T, scale):
    s = torch.randn(G, T, T, generator=_g(G + T)) * 4
    want, bar = _bar(lambda a: R.softmax_columns(a, scale)[0], s)
    ref = F.softmax(s.double() * scale, dim=1)
    err = float((want - ref).abs().max())
    print(f"softmax G={G} T={T} scale={scale}: |ref64 - F.softmax| = {err:.3e}, bar = {bar:.3e}")
    assert err <= bar                                      # measured: err <= 2.0e-15 against bars 0 (T = 1) .. 8.4e-7
    assert float((want.sum(1) - 1).abs().max()) < 1e-14


@pytest.mark.parametrize("heads,T", [(1, 7), (2, 33), (3, 129), (16, 64)])
def test_attention_is_the_oracle_self_attention(heads, T):
    dim, B = heads * 64, 2
    g = _g(heads + T)
    att = ow2._SelfAttention(dim, heads).double()
    q, k, v = (torch.randn(B, dim, T, generator=g) * s for s in (1.5, 1.5, 1.0))
    with torch.no_grad():
        att.out_proj.weight.copy_(torch.eye(dim, dtype=torch.float64))
        att.out_proj.bias.zero_()
        ref = _through(att, q, k, v)
    want, bar = _bar(lambda *a: R.attention(*a, heads, 64 ** -0.5)[0], q, k, v)
    err = float((want - ref).abs().max())
    print(f"attention heads={heads} T={T}: |ref64 - _SelfAttention| = {err:.3e}, bar = {bar:.3e}")
    assert want.shape == ref.shape and err <= bar          # measured: err <= 1.4e-15 against bars 1.2e-6 .. 5.3e-6
    a = R.attention(q, k, v, heads, 64 ** -0.5)[1]
    assert float((a["w"].sum(-1) - 1).abs().max()) < 1e-14 and float(a["gap2"].min()) == 0.0


def _through(att, q, k, v):
    """the oracle module on given q, k, v [B, C, T]: its three projections, which it applies to one input, are replaced by modules
    that hand out the given tensors"""
    class Pick(torch.nn.Module):
        def __init__(self, t):
            super().__init__()
            self.t = t

        def forward(self, x):
            return self.t

    saved = att.q_proj, att.k_proj, att.v_proj
    att.q_proj, att.k_proj, att.v_proj = (Pick(t.double().transpose(1, 2)) for t in (q, k, v))
    try:
        return att(torch.zeros(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float64)).transpose(1, 2)
    finally:
        att.q_proj, att.k_proj, att.v_proj = saved


@pytest.mark.parametrize("n,B", [(400, 1), (560, 3), (2011, 3), (8000, 2)])
@pytest.mark.parametrize("pad", (0, 19))
def test_fbank_is_the_oracle_fbank_with_cmvn_and_pad_input(n, B, pad):
    from satools_amd import synthetic
    wav = synthetic.harm_batch(list(range(B)), n) + 0.01 * torch.randn(B, n, generator=_g(n))
    window, mel = ofb.povey_window(), ofb.mel_banks(80)
    want, bar = _bar(lambda x: R.fbank(x, window, mel, scale=32768.0, cmvn=True, pad=pad)[0], wav)
    ref = ofb.fbank(wav * 32768, 80)
    ref = otd.pad_input(ref - ref.mean(dim=1).unsqueeze(1), pad).permute(0, 2, 1).double()
    err = float((want - ref).abs().max())
    print(f"fbank n={n} B={B} pad={pad}: |ref64 - oracle| = {err:.3e}, bar (2 x float32 error) = {bar:.3e}")
    assert want.shape == ref.shape == (B, 80, (n + 80) // 160 + 2 * pad)
    assert err <= bar, (err, bar)                          # measured: err 2.7e-6 .. 9.4e-5 against bars 4.8e-6 .. 1.9e-4 (n = 8000: quiet high mel bins)
    raw, _ = R.fbank(wav, window, mel, scale=32768.0, cmvn=False, pad=0)
    assert float((raw - ofb.fbank(wav * 32768, 80).permute(0, 2, 1).double()).abs().max()) <= bar
    # silence sits on the floor, and scale = 1 is the same features 2 log 32768 lower
    z = R.fbank(torch.zeros(1, n), window, mel, scale=1.0, cmvn=False)[0]
    assert bool((z == float(np.log(np.float64(np.float32(1e-6))))).all())
    one, a1 = R.fbank(wav, window, mel, scale=1.0, cmvn=False)
    above = a1["mel"] > 1e-6
    assert bool(above.any()) and float((raw - one - 2 * np.log(32768.0))[above].abs().max()) < 1e-9


def test_fbank_framing_and_padding_follow_their_definitions():
    w = torch.arange(1.0, 561.0).unsqueeze(0)
    fr = R.fbank_frames(w.double())
    assert fr.shape == (1, 4, 400)
    assert torch.equal(fr[0, 0, :121], torch.cat([torch.arange(120.0, 0.0, -1.0), torch.tensor([1.0])]).double())      # w[119..0], w[0]
    assert fr[0, 3, 198:202].tolist() == [559.0, 560.0, 560.0, 559.0] and float(fr[0, 3, -1]) == 361.0                 # .., w[n-1], w[n-1], ..
    assert torch.equal(fr.float(), ofb.frames(w[0]).unsqueeze(0))
    x = torch.randn(3, 5, 4, generator=_g(1)).double()
    assert torch.equal(R.pad_frames(x, 19), otd.pad_input(x.permute(0, 2, 1), 19).permute(0, 2, 1))
    assert R.pad_frames(x, 0) is x


# ---- the fast GELUs ------------------------------------------------------------------------------------------------------------------
def _fast_gelu_error(taylor):
    x = np.linspace(-8.0, 8.0, 2 ** 21 + 1).astype(np.float32)
    err = np.abs(R.gelu_fast_f32(x, taylor).astype(np.float64) - R.gelu(torch.from_numpy(x)).numpy())
    i = int(err.argmax())
    print(f"fast GELU ({'gelu_fast' if taylor else 'gelu_fast4'}): max |float32 formula - float64| on [-8, 8] = {err[i]:.4e} at x = {x[i]:.4f}")
    return float(err[i])


def test_gelu_fast4_error_is_the_stated_one():
    """csrc/common.h states 4.7e-7 for gelu_fast4 on [-8, 8]: the same float32 formula evaluated here (fused multiply-adds where the
    kernel has them, a correctly rounded reciprocal and exp2 in place of the device's 1-ULP ones) against float64 on a grid of 2 M points.
    Beyond 8 the result is x / 2 * 2 or * 0: one rounding.  And how an error of the argument reaches the result: max |GELU'|"""
    assert _fast_gelu_error(False) <= K.GELU_FAST4_ERR     # measured: 4.6998e-7 at x = 3.1273
    far = np.concatenate([np.linspace(-64.0, -8.0, 2 ** 16), np.linspace(8.0, 64.0, 2 ** 16)]).astype(np.float32)
    ex = R.gelu(torch.from_numpy(far)).numpy()
    assert bool((np.abs(R.gelu_fast_f32(far, False).astype(np.float64) - ex) <= K.GELU_FAST4_ERR + 2 * U * np.abs(ex)).all())
    xs = torch.linspace(-8, 8, 2 ** 20 + 1, dtype=torch.float64)
    slope = float(((R.gelu(xs[1:]) - R.gelu(xs[:-1])) / (xs[1:] - xs[:-1])).abs().max())
    assert 1.12 < slope <= K.GELU_SLOPE, slope              # 1.1290 at x = sqrt(2)


def test_gelu_fast_error_is_the_stated_one():
    """csrc/common.h states 3.6e-7 for gelu_fast.  As v / 2 * (1 + erf) — gelu_fast4's order of operations — the formula gave 4.6998e-7 at
    x = 3.1273, three roundings on top of the Abramowitz-Stegun error where that is largest; gelu_fast now forms the result from
    1 - erf(|z|) with one rounding (v - v / 2 * q e), and this float32 evaluation of that form is inside the stated figure"""
    assert _fast_gelu_error(True) <= K.GELU_FAST_ERR       # measured: 3.3292e-7 at x = 3.0663


# ---- the attention bound tells right from wrong ------------------------------------------------------------------------------------
def _attention_errors(case, variants):
    kind, heads, B, T, mode, scale = case
    q, k, v = K.attention_inputs(kind, B, heads, T, scale, K._gen(8, len(kind), heads, B, T))      # the GPU test's own inputs
    want, bound = K.attention_bound(q, k, v, heads, scale, K.P_SCALE_LOG2, subnormal=False)
    out = {}
    for var, ps in variants:
        err = (R.attention_split16(q, k, v, heads, scale, ps, var) - want).abs()
        out[(var, ps)] = (float((err / bound).max()), float(err.max()))
    return out


def test_split16_emulation_is_the_attention_up_to_the_split():
    q, k, v = K.attention_inputs("gaussian", 2, 3, 300, 0.125, _g(3))
    want, bound = K.attention_bound(q, k, v, 3, 0.125, 0, subnormal=True)
    assert torch.equal(want, R.attention(q, k, v, 3, 0.125)[0])
    for ps in (0, 10):
        err = (R.attention_split16(q, k, v, 3, 0.125, ps) - want).abs()
        print(f"split-f16 arithmetic, Gaussian inputs, T = 300, P x 2^{ps}: max error {float(err.max()):.2e}, error / bound {float((err / bound).max()):.3f}")
        assert float(err.max()) < 1e-5 and bool((err <= bound).all())     # the bar of test_hip_w2v2.py::test_fused_attention_matches_float64; measured 2.8e-6
    with pytest.raises(AssertionError):
        R.attention_split16(q, k, v, 3, 0.125, 0, "nonsense")


def test_attention_bound_holds_for_the_kernels_arithmetic_and_fails_four_wrong_kernels():
    """on every case of test_hip_w2v2_kernels.py::test_attention_fused the kernel's arithmetic (float64 sums, P times 2^10 before its
    split as in the kernel) stays inside the bound the GPU test uses; each of the four wrong kernels leaves it on at least one case of the
    adversarial set (every kind at every T edge, 2 heads, B = 1).  Also printed: the absolute error of the dominant-key cases with the
    weights split unscaled (p_scale_log2 = 0) and scaled"""
    wrong = [v for v in R.VARIANTS if v != "ok"]
    caught = {v: [] for v in wrong}
    worst_ok = (0.0, None)
    for case in K.attention_cases():
        kind, heads, B, T = case[:4]
        adversarial = (heads, B) == (2, 1)
        variants = [("ok", K.P_SCALE_LOG2)] + ([("ok", 0)] + [(v, K.P_SCALE_LOG2) for v in wrong] if adversarial else [])
        res = _attention_errors(case, variants)
        r, e = res[("ok", K.P_SCALE_LOG2)]
        assert r <= 1.0, (case, r, e)
        worst_ok = max(worst_ok, (r, case))
        if adversarial:
            if kind.startswith("dominant"):
                print(f"{kind} T={T} scale={case[5]}: |emulation - float64| unscaled P {res[('ok', 0)][1]:.2e}, P x 2^{K.P_SCALE_LOG2} {e:.2e}"
                      f" (error / bound {res[('ok', 0)][0]:.3f}, {r:.3f})")
            for v in wrong:
                if res[(v, K.P_SCALE_LOG2)][0] > 1.0:
                    caught[v].append((kind, T, round(res[(v, K.P_SCALE_LOG2)][0], 1)))
    print("largest error / bound of the right arithmetic:", worst_ok)
    for v in wrong:
        print(f"{v}: outside the bound on {len(caught[v])} cases, e.g. {caught[v][:4]}")
        assert caught[v], v
