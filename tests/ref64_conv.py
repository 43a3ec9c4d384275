"""Float64 restatement of sat_conv1d_desc (include/satools_hip.h): the pre-epilogue sum and the epilogue in the header's one order, with a
running error bound, and the lattice of option sets ops.conv1d exposes.  Plain torch on the CPU: no fixtures, no GPU.

    v = sum W pre(x) ; v += bias ; residual before the activation ; ReLU (relu_first) ; folded BatchNorm ; ReLU ; GELU ;
    residual after the activation (res_after_act) ; accum ; accum_div ; the f32 store and / or the split planes of lrelu(v, slope)

The bound starts at E0 = 3e-5 absolute, the project's bar for SAT_CONV_F32 and SAT_CONV_F16X3 on inputs randn and weights randn * fan_in^-1/2
(tests/test_hip_parity.py::test_conv1d_matches_torch, ::test_conv1d_split_f16_matches_torch, `bound` of conv_case in tests/test_hip_bounds.py), and
every epilogue step moves it by what one correctly rounded float32 operation (U = 2^-24) adds and by how the step passes an error on:

    residual            e + 2U(|v'| + |res_scale r|)              one rounding for the product, one for the sum; a residual rebuilt from
                                                                   SAT_SPLIT_F16 planes adds 2^-21 |r| (22 of its 24 bits)
    relu                e                                          1-Lipschitz, exact
    affine              e |sc| + 2U(|v'| + |sh|)
    gelu                1.13 e + GELU_FAST_ERR + 4U |v'|           max |GELU'| = 1.129; csrc/common.h gelu_fast: 3.6e-7 on [-8, 8]
    accum               e + U |v'|
    accum_div           e / |div| + U |v'|
    planes              e + 2^-21 |want|                           lrelu with a slope in [0, 1] is 1-Lipschitz; hi + lo carries 22 bits

(v' = the value after the step.)  tests/test_ref64_conv.py pins all of this; tests/test_hip_conv_options.py holds the kernels to it."""
import itertools
from typing import NamedTuple

import torch
import torch.nn.functional as F

from ref64 import U

E0 = 3e-5
GELU_FAST_ERR = 3.6e-7          # tests/test_hip_w2v2_kernels.py::test_conv_epilogue_gelu_fast
GELU_SLOPE = 1.13
SPLIT_RESIDUAL = 2.0 ** -21
Y_SLOPE = 0.1                   # y_split_slope and res_split_slope of every call of the matrix
IN_SLOPE = 0.1

_D = torch.float64


def _t(x, dt):
    return torch.as_tensor(x).detach().cpu().to(dt)


def _ch(v, dt):
    return _t(v, dt)[None, :, None]


# ---- the pre-epilogue sum ----------------------------------------------------------------------------------------------------------
def pre_sum(x, w, *, dilation=1, stride=1, pads=(0, 0), groups=1, in_slope=None, up=1, up_padding=0, wrap=0, t_q=None, dtype=_D):
    """sum_{ci, j} W pre(x), no bias.  x [B, C, T]: the f32 input, or for a call on split planes what ops.unsplit(x_split) gives (in_slope None).
    up == 1: w [C_out, C_in / groups, k] (torch Conv1d layout), `pads` = (left, right) zeros.
    up > 1:  w [C_in, C_out, k] is the ConvTranspose1d weight whose polyphase rows packing.convtranspose_as_phase_conv lays out (stride up,
             padding up_padding): the reference is F.conv_transpose1d itself.
    wrap:    x holds `wrap` channels and input channel c >= wrap reads channel c - wrap one position later (sat_conv1d_desc.x_wrap_channels)"""
    x, w = _t(x, dtype), _t(w, dtype)
    if in_slope is not None:
        x = F.leaky_relu(x, in_slope)
    if up > 1:
        assert stride == 1 and groups == 1 and not wrap
        return F.conv_transpose1d(x, w, stride=up, padding=up_padding)
    if wrap:
        nxt = F.pad(x[:, :w.shape[1] - wrap, 1:], (0, 1))
        return F.conv1d(x, w[:, :wrap]) + F.conv1d(nxt, w[:, wrap:])
    v = F.conv1d(F.pad(x, tuple(pads)), w, stride=stride, dilation=dilation, groups=groups)
    return v if t_q is None else v[..., :t_q]


# ---- the epilogue ------------------------------------------------------------------------------------------------------------------
def epilogue(s, *, bias=None, res=None, res_scale=1.0, res_toff=0, res_tstride=1, res_after=False, res_planes=False, ch_scale=None, ch_shift=None,
             relu=False, relu_first=False, gelu=False, y_old=None, accum_div=0.0, e0=E0, dtype=_D):
    """s [B, C_out, T] -> (want, bound) in the header's order.  res [B, C_out, >= (T - 1) res_tstride + res_toff + 1]: element t of the output
    takes res[t * res_tstride + res_toff] (t = q * up + phase: the index of the OUTPUT); res_planes: it reaches the kernel as SAT_SPLIT_F16 planes.
    y_old: the tensor `accum` adds to (None = no accumulation).  dtype=torch.float32 evaluates the same chain in float32 torch (the yardstick of
    tests/test_ref64_conv.py); the bound is always the float64 one of the float64 values."""
    dt = dtype
    v = _t(s, dt)
    T = v.shape[-1]
    vd = _t(s, _D)          # the float64 value next to it: the bound is built from exact magnitudes
    e = torch.full_like(vd, e0)

    def both(fn):
        nonlocal v, vd
        v = fn(v, dt)
        vd = v if dt == _D else fn(vd, _D)

    def add_res():
        nonlocal e
        r = res[..., res_toff::res_tstride][..., :T]
        both(lambda a, d: a + _t(r, d) * res_scale)          # (the descriptor's float res_scale is within U / 2 of this one: inside the step's 2U)
        rd = _t(r, _D).abs()
        e = e + 2 * U * (vd.abs() + abs(res_scale) * rd)
        if res_planes:
            e = e + SPLIT_RESIDUAL * rd

    if bias is not None:
        both(lambda a, d: a + _ch(bias, d))          # (inside E0: the bar of the parity tests is on conv + bias)
    if res is not None and not res_after:
        add_res()
    if relu and relu_first:
        both(lambda a, d: F.relu(a))
    if ch_scale is not None:
        both(lambda a, d: a * _ch(ch_scale, d) + _ch(ch_shift, d))
        e = e * _ch(ch_scale, _D).abs() + 2 * U * (vd.abs() + _ch(ch_shift, _D).abs())
    if relu and not relu_first:
        both(lambda a, d: F.relu(a))
    if gelu:
        both(lambda a, d: F.gelu(a))
        e = GELU_SLOPE * e + GELU_FAST_ERR + 4 * U * vd.abs()
    if res is not None and res_after:
        add_res()
    if y_old is not None:
        both(lambda a, d: _t(y_old, d)[..., :T] + a)
        e = e + U * vd.abs()
    if accum_div != 0.0:
        both(lambda a, d: a / accum_div)
        e = e / abs(accum_div) + U * vd.abs()
    return v, e


def planes(want, bound, slope=Y_SLOPE):
    """what ops.unsplit(y_split) must give: (lrelu(want, slope), bound + 2^-21 |that|)"""
    p = F.leaky_relu(want, slope)
    return p, bound + SPLIT_RESIDUAL * p.double().abs()


# ---- the lattice of option sets ----------------------------------------------------------------------------------------------------
BIAS = (True, False)
RES = ("none", "f32", "f32 strided", "post", "planes", "planes scaled")
ACT = ("none", "relu", "relu_first", "gelu")
AFFINE = (False, True)
ACCUM = ("none", "accum", "accum div", "div")
OUT = ("f32", "f32 + planes", "planes")
IN_LRELU = (False, True)
AXES = {"bias": BIAS, "res": RES, "act": ACT, "affine": AFFINE, "accum": ACCUM, "out": OUT, "in_lrelu": IN_LRELU}
RES_SCALE, RES_TOFF, RES_TSTRIDE, ACCUM_DIV = 0.66, 1, 2, 3.0


class Opt(NamedTuple):
    bias: bool
    res: str
    act: str
    affine: bool
    accum: str
    out: str
    in_lrelu: bool

    def __str__(self):
        return (f"bias {int(self.bias)} | res {self.res} | act {self.act} | affine {int(self.affine)} | accum {self.accum} | out {self.out} | "
                f"in_lrelu {int(self.in_lrelu)}")


def lattice(f32_input=True, **fixed):
    """every option set (in_lrelu only with an f32 input); `fixed` pins axes to one value"""
    axes = dict(AXES)
    if not f32_input:
        axes["in_lrelu"] = (False,)
    for k, v in fixed.items():
        axes[k] = (v,)
    return [Opt(*c) for c in itertools.product(*(axes[f] for f in Opt._fields))]


def value_key(o):
    """the part of an option set its VALUE depends on (`out` only picks the stores)"""
    return o._replace(out="f32")


class EpiInputs(NamedTuple):
    bias: torch.Tensor          # [C]
    ch_scale: torch.Tensor      # [C]  |randn| + 0.5
    ch_shift: torch.Tensor      # [C]  randn: non-zero
    res: torch.Tensor           # [B, C, 2 T + 2]: the f32 residual of every kind (the strided kind reads the odd elements)
    res_p: torch.Tensor         # [B, C, T]: the residual that travels as planes (other values: the two kinds can be told apart)
    y_old: torch.Tensor         # [B, C, T]


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def epilogue_inputs(B, C, T, seed=0):
    """O(1) operands of the epilogue, all float32: about half of conv + bias + residual is negative, the shift is non-zero"""
    return EpiInputs(_rand(C, seed=seed + 3), _rand(C, seed=seed + 9).abs() + 0.5, _rand(C, seed=seed + 10), _rand(B, C, 2 * T + 2, seed=seed + 4),
                     _rand(B, C, T, seed=seed + 6), _rand(B, C, T, seed=seed + 5))


def epilogue_kwargs(o, e):
    """an option set as the keyword arguments of `epilogue`"""
    kw = {}
    if o.bias:
        kw["bias"] = e.bias
    if o.res in ("f32", "post"):
        kw.update(res=e.res, res_after=o.res == "post")
    elif o.res == "f32 strided":
        kw.update(res=e.res, res_scale=RES_SCALE, res_toff=RES_TOFF, res_tstride=RES_TSTRIDE)
    elif o.res in ("planes", "planes scaled"):
        kw.update(res=e.res_p, res_planes=True, res_scale=RES_SCALE if o.res == "planes scaled" else 1.0)
    if o.act != "none":
        kw.update(relu=o.act in ("relu", "relu_first"), relu_first=o.act == "relu_first", gelu=o.act == "gelu")
    if o.affine:
        kw.update(ch_scale=e.ch_scale, ch_shift=e.ch_shift)
    if o.accum in ("accum", "accum div"):
        kw["y_old"] = e.y_old
    if o.accum in ("accum div", "div"):
        kw["accum_div"] = ACCUM_DIV
    return kw


def conv(s, o, e, dtype=_D):
    """(want, bound) of option set `o` on the pre-epilogue sum `s` (of pre_sum, with or without the input leaky-relu as o.in_lrelu says)"""
    return epilogue(s, dtype=dtype, **epilogue_kwargs(o, e))


def equivalent(a, b):
    """the reason two option sets that differ in one option have the same value, or None"""
    diff = [f for f in Opt._fields if getattr(a, f) != getattr(b, f)]
    assert len(diff) == 1, diff
    f, (va, vb) = diff[0], sorted((getattr(a, diff[0]), getattr(b, diff[0])))
    for rule in EQUIVALENT:
        if rule["axis"] == f and (va, vb) == tuple(sorted(rule["values"])) and rule["when"](a):
            return rule["reason"]
    return None


EQUIVALENT = [
    {"axis": "out", "values": v, "when": lambda o: True, "reason": "the output option picks the stores, not the value"}
    for v in itertools.combinations(OUT, 2)] + [
    {"axis": "act", "values": ("relu", "relu_first"), "when": lambda o: not o.affine, "reason": "relu_first only moves the ReLU across the affine step"},
    {"axis": "res", "values": ("f32", "post"), "when": lambda o: o.act == "none" and not o.affine,
     "reason": "nothing stands between the two places of the residual add"},
]
