"""Float64 restatements of the operations of the two ASR front ends: the wav2vec2 support kernels (csrc/w2v2.hip: first conv layer,
LayerNorm over channels with GELU and the even | odd phase split, softmax over the keys of a transposed score matrix, self-attention) and
the Kaldi fbank with per-utterance CMVN and the reference's padding (csrc/fbank.hip).

Written from the formulas, in float64 torch on the CPU, in the style of tests/ref64.py (whose U, in_float32() and f32() are used here): a
function whose result involves a reduction also returns, in a dict, the sums of absolute terms a rounding-error bound needs (S = sum |term|).
`attention_split16` is not a restatement of the operation but of the KERNEL's arithmetic (split-f16 operands, three products, keys in blocks
of 256 under a running maximum) with float64 sums, and can be made wrong in four deliberate ways: tests/test_ref64_w2v2.py uses it to show
that the error bound of tests/test_hip_w2v2_kernels.py tells a right kernel from a wrong one.  A plain module: no fixtures, no GPU.
tests/test_ref64_w2v2.py pins these functions against independent CPU computations."""
import math

import torch

import ref64
import ref_split16
from ref64 import U, f32  # noqa: F401  (re-exported)

LOG2E = 1.44269504088896340736
KEY_BLOCK = 256         # keys per block of the running softmax
VARIANTS = ("ok", "drop_hi_lo", "mask_off_by_one", "no_alpha_on_o", "v_lo_zero_last_block")


def _d(x):
    return ref64._d(x)


def _dt():
    return ref64._DT


# ---- wav2vec2: first conv layer, LayerNorm, softmax --------------------------------------------------------------------------------
def conv0(x, w, bias, stride):
    """x [B, n], w [C, k], bias [C] -> y [B, C, T], T = (n - k) // stride + 1: y[b, c, t] = bias[c] + sum_j w[c, j] x[b, t stride + j].
    aux: S = |bias| + sum_j |w x|"""
    x, w, bias = _d(x), _d(w), _d(bias)
    k = w.shape[1]
    win = x.unfold(1, k, stride)                                         # [B, T, k]
    y = bias.view(1, -1, 1) + torch.einsum("btj,cj->bct", win, w)
    S = bias.abs().view(1, -1, 1) + torch.einsum("btj,cj->bct", win.abs(), w.abs())
    return y, {"S": S}


def gelu(v):
    """the exact (erf) GELU"""
    v = _d(v)
    return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))


def phase_split(y):
    """[B, C, T] -> [B, 2 C, ceil(T / 2)]: the even frames | the odd frames, the odd half's last slot zero for an odd T"""
    B, C, T = y.shape
    out = torch.zeros(B, 2 * C, (T + 1) // 2, dtype=y.dtype)
    out[:, :C] = y[:, :, 0::2]
    out[:, C:, :T // 2] = y[:, :, 1::2]
    return out


def layernorm_channels(x, gamma, beta, eps=1e-5, gelu_after=False, split_phases=False):
    """x [B, C, T]: (x - mean_c) / sqrt(biased var_c + eps) * gamma + beta over the channel axis, eps as float32; then optionally the exact
    GELU and the phase split.  aux (all in x's layout [B, C | 1, T]): S1 = sum |x|, S2 = sum (x - mean)^2, mean, var, d = x - mean,
    pre = the affine result before GELU and split"""
    x, gamma, beta = _d(x), _d(gamma).view(1, -1, 1), _d(beta).view(1, -1, 1)
    C = x.shape[1]
    mean = x.sum(1, keepdim=True) / C
    d = x - mean
    S2 = (d * d).sum(1, keepdim=True)
    var = S2 / C
    pre = d / torch.sqrt(var + f32(eps)) * gamma + beta
    y = gelu(pre) if gelu_after else pre
    if split_phases:
        y = phase_split(y)
    return y, {"S1": x.abs().sum(1, keepdim=True), "S2": S2, "mean": mean, "var": var, "d": d, "pre": pre}


def softmax_columns(st, scale):
    """st [G, T (key j), T (query)]: softmax over the keys of scale * st, for every (group, query column).
    aux: arg = scale * st - its column maximum (<= 0), prod = scale * st"""
    st = _d(st)
    prod = st * f32(scale)
    arg = prod - prod.max(1, keepdim=True).values
    e = torch.exp(arg)
    return e / e.sum(1, keepdim=True), {"arg": arg, "prod": prod}


# ---- self-attention -----------------------------------------------------------------------------------------------------------------
def _heads(t, heads):
    B, C, T = t.shape
    return t.reshape(B, heads, C // heads, T)


def attention(q, k, v, heads, scale):
    """q, k, v [B, heads * D, T] -> o [B, heads * D, T]: softmax_j(scale sum_c q[c, i] k[c, j]) v[d, j] per head.
    aux: "w" the softmax weights [B, H, T (query), T (key)], "gap2" = (max_j s - s) scale log2(e) >= 0 (the weights are 2^-gap2 / sum),
    "S_qk" = sum_c |q k| like gap2, "S_pv" = sum_j w |v| [B, H, D, T]"""
    qh, kh, vh = (_heads(_d(t), heads) for t in (q, k, v))
    s = torch.einsum("bhci,bhcj->bhij", qh, kh)
    S_qk = torch.einsum("bhci,bhcj->bhij", qh.abs(), kh.abs())
    a = s * f32(scale)
    gap = a.max(-1, keepdim=True).values - a
    e = torch.exp(-gap)
    w = e / e.sum(-1, keepdim=True)
    o = torch.einsum("bhij,bhdj->bhdi", w, vh)
    S_pv = torch.einsum("bhij,bhdj->bhdi", w, vh.abs())
    B, C, T = q.shape
    return o.reshape(B, C, T), {"w": w, "gap2": gap * LOG2E, "S_qk": S_qk, "S_pv": S_pv}


def split_halves(x):
    """float32 -> (hi, lo, residual) float64: the kernel's split of an operand (both halves rounded toward zero to f16, subnormals kept)
    and what the two halves leave out, x - hi - lo"""
    x = torch.as_tensor(x).to(torch.float32)
    hi, lo = ref_split16.split_activation(x)
    return hi, lo, x.double() - hi - lo


def attention_split16(q, k, v, heads, scale, p_scale_log2=0, variant="ok"):
    """The arithmetic of attention_f16x3_kernel with float64 sums.  Q, K, V and the weights P are each split by
    ref_split16.f16_toward_zero into hi + lo; a product is hi hi + hi lo + lo hi (first operand K resp. V, second Q resp. P); keys go in
    blocks of 256 under a running maximum (in log2 units) and sum, O and the sum rescaled by alpha = 2^(old max - new max) per block;
    P = 2^(scale log2(e) s - max + p_scale_log2) is rounded to float32 before its split and summed unsplit; O / sum at the end.
    variant: "ok", or one of four wrong kernels —
      "drop_hi_lo"            the hi lo product (K hi Q lo, V hi P lo) is left out
      "mask_off_by_one"       the key mask is `jk <= T`: key T (a zero row of K and of V) takes part in the softmax
      "no_alpha_on_o"         alpha rescales the running sum but not O
      "v_lo_zero_last_block"  the lo halves of V are zero in the last key block
    Returns o [B, heads * D, T] float64."""
    assert variant in VARIANTS, variant
    B, C, T = q.shape
    qh, ql, _ = (_heads(t, heads) for t in split_halves(q))
    kh, kl, _ = (_heads(t, heads) for t in split_halves(k))
    vh, vl, _ = (_heads(t, heads) for t in split_halves(v))
    ein = lambda a, b: torch.einsum("bhcj,bhci->bhij", a, b)             # [B, H, query i, key j]
    s = ein(kl, qh) + ein(kh, qh)
    if variant != "drop_hi_lo":
        s = s + ein(kh, ql)
    scale2 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    nkb = (T + KEY_BLOCK - 1) // KEY_BLOCK
    D = C // heads
    o = torch.zeros(B, heads, D, T, dtype=torch.float64)
    m_run = torch.full((B, heads, T, 1), -math.inf, dtype=torch.float64)
    l_run = torch.zeros(B, heads, T, 1, dtype=torch.float64)
    for kb in range(nkb):
        j0, j1 = kb * KEY_BLOCK, min(T, (kb + 1) * KEY_BLOCK)
        sb, vhb, vlb = s[..., j0:j1], vh[..., j0:j1], vl[..., j0:j1]
        if variant == "mask_off_by_one" and j1 == T and T % KEY_BLOCK:      # key T lies in this block: score 0, V row 0
            sb = torch.cat([sb, torch.zeros(B, heads, T, 1, dtype=torch.float64)], -1)
            vhb = torch.cat([vhb, torch.zeros(B, heads, D, 1, dtype=torch.float64)], -1)
            vlb = torch.cat([vlb, torch.zeros(B, heads, D, 1, dtype=torch.float64)], -1)
        if variant == "v_lo_zero_last_block" and kb == nkb - 1:
            vlb = torch.zeros_like(vlb)
        mx = torch.maximum(m_run, sb.max(-1, keepdim=True).values * scale2)
        alpha = torch.exp2(m_run - mx)                                   # 0 on the first block
        p = torch.exp2(sb * scale2 - mx + p_scale_log2).float()          # the kernel's P is a float32
        ph = ref_split16.f16_toward_zero(p)
        pl = ref_split16.f16_toward_zero(p - ph).double()
        ph = ph.double()
        l_run = l_run * alpha + p.double().sum(-1, keepdim=True)
        pv = torch.einsum("bhdj,bhij->bhdi", vlb, ph) + torch.einsum("bhdj,bhij->bhdi", vhb, ph)
        if variant != "drop_hi_lo":
            pv = pv + torch.einsum("bhdj,bhij->bhdi", vhb, pl)
        if variant != "no_alpha_on_o":
            o = o * alpha.transpose(2, 3)
        o = o + pv
        m_run = mx
    return (o / l_run.transpose(2, 3)).reshape(B, C, T)


# ---- Kaldi fbank, CMVN, padding -----------------------------------------------------------------------------------------------------
FB_WIN, FB_SHIFT, FB_NFFT = 400, 160, 512


def fbank_frames(wav):
    """wav [B, n] -> [B, m, 400], m = (n + 80) // 160: frames every 160 samples of [w[119..0], w, w[n-1..0]] (snip_edges=False)"""
    B, n = wav.shape
    assert n >= FB_WIN
    m = (n + FB_SHIFT // 2) // FB_SHIFT
    pad = FB_WIN // 2 - FB_SHIFT // 2
    padded = torch.cat([torch.flip(wav[:, :pad], [1]), wav, torch.flip(wav, [1])], 1)
    return padded.unfold(1, FB_WIN, FB_SHIFT)[:, :m]


def pad_frames(x, pad):
    """x [B, C, m] -> [B, C, m + 2 pad]: the first frame `pad` times on the left; on the right the reference's pad_input: frame p is
    the last frame of utterance (b pad + p) mod B"""
    if pad <= 0:
        return x
    B = x.shape[0]
    src = (torch.arange(B).unsqueeze(1) * pad + torch.arange(pad).unsqueeze(0)) % B        # [B, pad]
    right = x[:, :, -1][src].permute(0, 2, 1)
    return torch.cat([x[:, :, :1].expand(-1, -1, pad), x, right], 2)


def fbank(wav, window, mel, scale=32768.0, cmvn=True, pad=0, floor=1e-6, coef=0.97):
    """wav [B, n], window [400], mel [n_mel, 257] -> [B, n_mel, m + 2 pad]: every frame of `scale * wav` has its mean removed, is
    pre-emphasised (x[j] - coef x[j-1], x[-1] := x[0]; coef as float32) and windowed; 512-point rfft, |X|^2, the mel product,
    log(max(., floor as float32)); then the mean over the frames of every (utterance, mel) row is subtracted (cmvn) and the frames padded.
    aux: "mel" [B, n_mel, m] the mel sums before the floor, "raw" their floored log, "A" [B, m] = sum |windowed sample|,
    "amp" = |X| and "power" [B, m, 257], and what the input-side roundings scale with: "xs" = |scaled sample|, "d" = |sample - mean|,
    "pre" = |pre-emphasised| [B, m, 400], "absmean" [B, m] = sum |scaled sample| / 400"""
    wav, window, mel = _d(wav), _d(window), _d(mel)
    fr = fbank_frames(wav * f32(scale))
    d = fr - fr.sum(2, keepdim=True) / FB_WIN
    prev = torch.cat([d[:, :, :1], d[:, :, :-1]], 2)
    pre = d - f32(coef) * prev
    xw = pre * window
    X = torch.fft.rfft(torch.nn.functional.pad(xw, (0, FB_NFFT - FB_WIN)), dim=2)
    power = X.real ** 2 + X.imag ** 2
    melsum = torch.matmul(power, mel.t()).transpose(1, 2)               # [B, n_mel, m]
    raw = torch.log(melsum.clamp(min=f32(floor)))
    out = raw - raw.sum(2, keepdim=True) / raw.shape[2] if cmvn else raw
    aux = {"mel": melsum, "raw": raw, "A": xw.abs().sum(2), "amp": X.abs(), "power": power, "xs": fr.abs(), "d": d.abs(), "pre": pre.abs(),
           "absmean": fr.abs().sum(2) / FB_WIN}
    return pad_frames(out, pad), aux


# ---- the fast GELUs of csrc/common.h in float32 numpy (the device's v_rcp_f32 / v_exp_f32 replaced by correctly rounded ones) --------
def gelu_fast_f32(x, taylor_branch):
    """erf by Abramowitz-Stegun 7.1.26 in float32.  gelu_fast4 (taylor_branch=False): that branch alone, as v / 2 * (1 + erf).  gelu_fast:
    v - v / 2 * (1 - erf) above |z| = 0.6 (v / 2 * (1 - erf) for v < 0), the odd Taylor polynomial of erf below"""
    import numpy as np
    F = np.float32
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(F)      # one rounding (the product is exact in float64)
    x = np.asarray(x, dtype=F)
    z = x * F(0.70710678118654752440)
    az = np.abs(z)
    t = F(1.0) / fma(az, F(0.3275911), F(1.0))
    q = fma(t, F(1.061405429), F(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        q = fma(q, t, F(c))
    q = q * t
    z2 = z * z
    e = np.exp2((z2 * F(-1.4426950408889634)).astype(np.float64)).astype(F)
    h = x * F(0.5)
    if not taylor_branch:                                                 # gelu_fast4: v / 2 * (1 + erf)
        return h * (np.copysign(fma(-q, e, F(1.0)), z) + F(1.0))
    qe = q * e                                                            # gelu_fast: from 1 - erf(|z|) itself, one rounding in the fma
    big = np.where(x >= 0, fma(-h, qe, x), h * qe)
    s = fma(z2, F(-0.0008548327023450853), F(0.005223977625442188))
    for c in (-0.026866170645131252, 0.11283791670955126, -0.37612638903183754, 1.1283791670955126):
        s = fma(s, z2, F(c))
    s = s * z
    return np.where(az < F(0.6), h * (F(1.0) + s), big)
