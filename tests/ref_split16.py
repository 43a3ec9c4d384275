"""The split-f16 arithmetic of sat_conv2d_f16x3_f32 (include/satools_hip_conv2d16.h) emulated on the CPU: the SAME split of both operands
and the SAME three products per term, summed in float64 instead of the kernel's f32 — so what separates this from the kernel is the f32
accumulation alone, and what separates it from tests/ref64_resnet.conv2d is the split alone (the dropped lo * lo product and the
rounding of the lo halves).  A plain module: no fixtures, no GPU.

  activations   hi = f16(x), lo = f16(x - hi), both rounded TOWARD ZERO with f16 subnormals kept (v_cvt_pkrtz_f16_f32)
  weights       w' = w 2^e with the largest |w'| in [2^9, 2^10); hi = f16(w'), lo = f16(w' - hi), round to nearest (torch), as
                ops.pack_conv2d_weight_f16x3 does it
  a product     w_lo x_hi + w_hi x_lo + w_hi x_hi (each exact in float64: 11 x 11 bits), the sum times 2^-e"""
import math

import torch
import torch.nn.functional as F

import ref64_resnet

TARGET_EXP = 10
SPLIT_LIMIT = 65520.0


def f16_toward_zero(v):
    """float32 tensor -> the float32 value of f16(v) rounded toward zero (|v| < 65 520; f16 subnormals kept)"""
    v = v.to(torch.float32).contiguous()
    normal = (v.view(torch.int32) & ~0x1FFF).view(torch.float32)                      # 13 of the 23 fraction bits dropped
    sub = torch.trunc(v.double() * 2.0 ** 24).mul(2.0 ** -24).float()               # below 2^-14: multiples of 2^-24
    return torch.where(v.abs() < 2.0 ** -14, sub, normal)


def split_activation(x):
    """float32 -> (hi, lo) float64 tensors"""
    x = x.to(torch.float32)
    assert bool((x.abs() < SPLIT_LIMIT).all()), "outside the range of the split"
    hi = f16_toward_zero(x)
    lo = f16_toward_zero(x - hi)                                                     # (x - hi is exact in float32)
    return hi.double(), lo.double()


def scale_exponent(w):
    m = float(w.abs().max())
    return 0 if m == 0.0 else max(-100, min(100, TARGET_EXP - math.frexp(m)[1]))


def split_weight(w):
    """float32 -> (hi, lo float64 of w 2^e, e)"""
    e = scale_exponent(w)
    p = w.to(torch.float32) * float(2.0 ** e)
    hi = p.to(torch.float16)
    lo = (p - hi.float()).to(torch.float16)
    return hi.double(), lo.double(), e


def conv2d(x, w, stride=1, scale=None, shift=None, relu=False):
    """ref64_resnet.conv2d's contract in split-f16 arithmetic.  x is rounded to float32 first (the kernel's input is float32)"""
    xh, xl = split_activation(torch.as_tensor(x).to(torch.float32))
    wh, wl, e = split_weight(torch.as_tensor(w))
    pad = w.shape[2] // 2
    conv = lambda a, b: F.conv2d(a, b, None, stride=stride, padding=pad)
    s = (conv(xh, wl) + conv(xl, wh) + conv(xh, wh)) * float(2.0 ** -e)
    v = s
    if scale is not None:
        v = s * torch.as_tensor(scale).double().view(1, -1, 1, 1) + torch.as_tensor(shift).double().view(1, -1, 1, 1)
    return torch.relu(v) if relu else v


def forward(sd, feats):
    """ref64_resnet.forward with every conv of the residual blocks (3x3 and 1x1 shortcuts) in the emulated split-f16 arithmetic; the stem
    and everything else as there.  Returns (x_vector [B, 256], taps)"""
    inner = ref64_resnet.conv2d

    def routed(x, w, stride=1, scale=None, shift=None, relu=False):
        if w.shape[1] == 1:                                                          # the stem stays exact
            return inner(x, w, stride, scale, shift, relu)
        return conv2d(x, w, stride, scale, shift, relu), {}

    ref64_resnet.conv2d = routed
    try:
        return ref64_resnet.forward(sd, feats)
    finally:
        ref64_resnet.conv2d = inner
