"""Float64 restatements of the small operations around the convolutions: the x-vector front end and pooling
(sidekit/preprocessor.py MelSpecFrontEnd, augmentation.py PreEmphasis, sidekit/nn.py SE gate, pooling.py
AttentiveStatsPool, F.normalize), the F0 transforms (cmvn.py UttCMVN keep_zeros, hifigan/nn.py quantize_f0 /
awgn_f0 / mean_reverv_f0), the generator-input assembly and the ASR-side padding and log-softmax.

Written from the reference's formulas, in float64 torch on the CPU.  A function whose result involves a reduction
also returns, in a dict, the sums of absolute terms a rounding-error bound needs (S = sum |term|).  Inputs are
float32 tensors (or anything torch.as_tensor takes); constants the reference holds as float32 (the pre-emphasis
coefficient, the 1/n averaging window) enter as their float32 values.  A plain module: no fixtures, no GPU.
tests/test_ref64.py pins these functions against the reference's own outputs."""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of float32: one correctly rounded operation has relative error <= U


_DT = torch.float64


def _d(x):
    return torch.as_tensor(x).detach().cpu().to(_DT)


@contextlib.contextmanager
def in_float32():
    """evaluate the same formulas in float32 torch on the CPU: how far float32 arithmetic strays from them is the yardstick
    tests/test_ref64.py measures its bars with"""
    global _DT
    _DT = torch.float32
    try:
        yield
    finally:
        _DT = torch.float64


def f32(v):
    """the float32 nearest to the Python float v, as a Python float"""
    return float(np.float32(v))


# ---- x-vector front end ----------------------------------------------------------------------------------------------
def pre_emphasis(x, coef=0.97):
    """[B, n]: y[t] = x[t] - coef * x[t-1], x[-1] := x[1] (reflect pad of one sample); coef as float32"""
    x = _d(x)
    prev = torch.cat([x[:, 1:2] if x.shape[1] > 1 else x[:, :1], x[:, :-1]], dim=1)
    return x - f32(coef) * prev


def melspec(wav, window, fb, coef=0.97, n_fft=1024, hop=160):
    """wav [B, n], window [win], fb [n_mel, n_fft/2+1] -> mel power [B, n_mel, 1 + n // hop] BEFORE the `+ 1e-6` and the log,
    by a direct float64 rfft of every frame of the reflect-padded (n_fft/2 a side, torch.stft center=True), pre-emphasised
    signal, the window centred in the n_fft frame.
    aux: "A" [B, frames] = sum |windowed sample| of the frame (every |X_k| and every FFT rounding error scales with it),
         "power" [B, frames, n_fft/2+1], "amp" = |X| [B, frames, n_fft/2+1]"""
    y = pre_emphasis(wav, coef)
    window, fb = _d(window), _d(fb)
    B, n = y.shape
    if n <= n_fft // 2:
        raise ValueError("reflect padding needs more than n_fft/2 samples")
    yp = F.pad(y.unsqueeze(1), (n_fft // 2, n_fft // 2), mode="reflect").squeeze(1)
    frames = yp.unfold(1, n_fft, hop)                                    # [B, 1 + n // hop, n_fft]
    assert frames.shape[1] == 1 + n // hop
    wfull = torch.zeros(n_fft, dtype=_DT)
    off = (n_fft - window.numel()) // 2
    wfull[off:off + window.numel()] = window
    xw = frames * wfull
    X = torch.fft.rfft(xw, dim=2)
    power = X.real ** 2 + X.imag ** 2
    mel = torch.matmul(power, fb.t()).transpose(1, 2)                    # [B, n_mel, frames]
    return mel, {"A": xw.abs().sum(2), "power": power, "amp": X.abs()}


def logmel(wav, window, fb, coef=0.97):
    return torch.log(melspec(wav, window, fb, coef)[0] + f32(1e-6))


def instance_norm(x, eps=1e-5):
    """rows along the last axis: (x - mean) / sqrt(biased var + eps).  aux: S1 = sum |x|, S2 = sum (x - mean)^2, mean, var"""
    x = _d(x)
    T = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / T
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / T
    y = d / torch.sqrt(var + f32(eps))
    return y, {"S1": x.abs().sum(-1, keepdim=True), "S2": (d * d).sum(-1, keepdim=True), "mean": mean, "var": var}


def row_mean(x):
    x = _d(x)
    return x.sum(-1, keepdim=True) / x.shape[-1], {"S1": x.abs().sum(-1, keepdim=True)}


def add3(a, b, c=None):
    y = _d(a) + _d(b)
    return y if c is None else y + _d(c)


def se_gate_add(z, gate_logits, skips=()):
    """z [B, C, T] * sigmoid(g [B, C]) + skips[0] + skips[1] + ...
    aux: "prod" = |z * gate|, "partials" = sum of |partial sum| after each add (every add rounds its own result)"""
    z, g = _d(z), _d(gate_logits).reshape(z.shape[0], z.shape[1], 1)
    gate = torch.sigmoid(g)
    v = z * gate
    prod = v.abs()
    partials = torch.zeros_like(v)
    for s in skips:
        v = v + _d(s)
        partials = partials + v.abs()
    return v, {"prod": prod, "partials": partials, "gate": gate}


def tanh(x):
    return torch.tanh(_d(x))


def attentive_stats(x, logits):
    """[B, C, T] x 2: w = softmax_t(logits); mean = sum w x; std = sqrt(max(sum w x^2 - mean^2, 1e-9)) (the reference's formula).
    Returns (mean [B, C], std [B, C], aux): "m2", "var" (unclamped), S1 = sum |w x|, S2 = sum w x^2, and the sums a bound on the
    softmax weights needs: E1 = sum |w x| (max - logit), E2 = sum w x^2 (max - logit), Ew = sum w (max - logit)"""
    x, l = _d(x), _d(logits)
    mx = l.max(-1, keepdim=True).values
    gap = mx - l
    w = torch.softmax(l, dim=-1)
    wx, wx2 = w * x, w * x * x
    mean, m2 = wx.sum(-1), wx2.sum(-1)
    var = m2 - mean * mean
    std = torch.sqrt(var.clamp(min=f32(1e-9)))
    aux = {"m2": m2, "var": var, "S1": wx.abs().sum(-1), "S2": wx2.sum(-1), "E1": (wx.abs() * gap).sum(-1), "E2": (wx2 * gap).sum(-1),
           "Ew": (w * gap).sum(-1)}
    return mean, std, aux


def l2norm(x):
    """rows of [R, D] / max(||row||, 1e-12).  aux: S = sum x^2, nrm"""
    x = _d(x)
    s = (x * x).sum(-1, keepdim=True)
    nrm = torch.sqrt(s)
    return x / nrm.clamp(min=1e-12), {"S": s, "nrm": nrm}


# ---- F0 --------------------------------------------------------------------------------------------------------------
def f0_stats(f0):
    """over the non-zero entries of the whole tensor: (mean, sqrt(unbiased var + 1e-6)); NaN like torch for none / one voiced value.
    aux: count, S1 = sum |v|, S2 = sum (v - mean)^2"""
    x = _d(f0).reshape(-1)
    v = x[x != 0]
    cnt = v.numel()
    nan = float("nan")
    mean = v.sum() / cnt if cnt else torch.tensor(nan, dtype=_DT)
    d = v - mean
    var = (d * d).sum() / (cnt - 1) if cnt > 1 else torch.tensor(nan, dtype=_DT)
    return mean, torch.sqrt(var + f32(1e-6)), {"count": cnt, "S1": v.abs().sum(), "S2": (d * d).sum(), "var": var}


def f0_normalise(f0):
    """(x - mean) / std on the non-zero entries, zeros stay zero"""
    x = _d(f0)
    mean, std, aux = f0_stats(x)
    return torch.where(x != 0, (x - mean) / std, torch.zeros_like(x)), dict(aux, mean=mean, std=std)


def f0_quantise(x, bins):
    """round(x * bins) / bins (half to even, torch.round), zeros stay zero"""
    x = _d(x)
    return torch.where(x != 0, torch.round(x * bins) / bins, torch.zeros_like(x))


def f0_awgn(x, noise):
    """x + noise where x != 0, zeros stay zero"""
    x = _d(x)
    return torch.where(x != 0, x + _d(noise), torch.zeros_like(x))


def mean_reversion(f0, alpha, n):
    """f0 [..., T] -> (1 - alpha) * f0 + alpha * avg, avg[t] = w * sum_k f0[t - n // 2 + k], k = 0 .. n - 1 (zeros outside),
    w = float32(1 / n) (the reference's window tensor `torch.ones(n) / n`), alpha and 1 - alpha as float32.
    aux: S = w * sum |f0| over the window, avg"""
    x = _d(f0)
    T = x.shape[-1]
    w = float(np.float32(1.0) / np.float32(n))
    lo = n // 2
    xp = F.pad(x, (lo, n - 1 - lo))                                      # window of output t = xp[t .. t + n - 1]
    win = xp.unfold(-1, n, 1)
    avg = w * win.sum(-1)
    S = w * win.abs().sum(-1)
    a, oma = f32(alpha), f32(1.0 - float(alpha))
    return oma * x + a * avg, {"S": S, "avg": avg, "alpha": a, "one_minus_alpha": oma}


# ---- generator input, ASR side ---------------------------------------------------------------------------------------
def nearest_interpolate(f0, T):
    """[B, T_f0] -> [B, T]: torch's own CPU F.interpolate(mode="nearest") on float32 (the index choice is integer-exact: no float64 restatement)"""
    x = torch.as_tensor(f0).detach().cpu().to(torch.float32)
    return F.interpolate(x.unsqueeze(1), size=T, mode="nearest").squeeze(1)


def assemble_input(bn, f0, spk):
    """cat(bn [B, C, T], nearest-interpolated f0 [B, 1, T], spk [B, n_spk] broadcast over T) in float32 (a pure selection)"""
    bn = torch.as_tensor(bn).detach().cpu().to(torch.float32)
    B, _, T = bn.shape
    parts = [bn, nearest_interpolate(torch.as_tensor(f0).reshape(B, -1), T).unsqueeze(1)]
    if spk is not None and spk.numel():
        parts.append(torch.as_tensor(spk).detach().cpu().to(torch.float32).reshape(B, -1, 1).expand(-1, -1, T))
    return torch.cat(parts, dim=1)


def pad_replicate(x, left, right, interleave_right=False):
    """[B, C, T] -> [B, C, left + T + right] in float32.  Left: the first frame repeated.  Right: the last frame repeated
    (F.pad(mode="replicate")), or with `interleave_right` the reference's pad_input: the last frames of the B utterances tiled as
    one sequence and cut into B pieces, so right-pad frame p of utterance b is the last frame of utterance (b * right + p) mod B"""
    x = torch.as_tensor(x).detach().cpu().to(torch.float32)
    B = x.shape[0]
    if not interleave_right:
        return F.pad(x, (left, right), mode="replicate")
    y = F.pad(x, (left, 0), mode="replicate")
    if right == 0:
        return y
    last = x[:, :, -1]                                                   # [B, C]
    src = (torch.arange(B).unsqueeze(1) * right + torch.arange(right).unsqueeze(0)) % B      # [B, right]
    return torch.cat([y, last[src].permute(0, 2, 1)], dim=2)


def log_softmax_channels(x):
    """log-softmax over axis 1 of [B, C, T].  aux: lse [B, 1, T], logtot = log sum exp(x - max), E = sum softmax * (max - x)"""
    x = _d(x)
    m = x.max(1, keepdim=True).values
    tot = torch.exp(x - m).sum(1, keepdim=True)
    lse = m + torch.log(tot)
    p = torch.exp(x - lse)
    return x - lse, {"lse": lse, "logtot": torch.log(tot), "E": (p * (m - x)).sum(1, keepdim=True)}


def tdnnf_unfold15(x):
    """x [B, D, T] -> (windows, bypass) [B, D, (2 (T - 1)) // 3 + 1] of a TDNNF layer with subsampling 1.5 (chain/nn.py): the
    flattened frame-major [T * D] sequence cut into windows of D values every int(1.5 D); the bypass takes frames 0, 1, 3, 4, 6, 7,
    ... for the first int(T / 1.5) windows, zero after.  float32, a pure selection"""
    x = torch.as_tensor(x).detach().cpu().to(torch.float32)
    B, D, T = x.shape
    Tq = (2 * (T - 1)) // 3 + 1
    flat = x.permute(0, 2, 1).reshape(B, T * D)
    step = int(1.5 * D)
    win = torch.stack([flat[:, k * step:k * step + D] for k in range(Tq)], dim=2)
    byp = torch.zeros(B, D, Tq)
    for k in range(min(Tq, (2 * T) // 3)):
        byp[:, :, k] = x[:, :, (3 * k) // 2]
    return win, byp


def reduction_terms(n, lanes=64, extra=8):
    """roundings a sum of n terms collects on one wave: ceil(n / lanes) sequential adds per lane, six shuffle levels and the
    multiply / divide around it (extra = 8)"""
    return math.ceil(n / lanes) + extra
