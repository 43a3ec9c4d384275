"""The small HIP kernels around the convolutions (csrc/xvector.hip, bottleneck.hip, fbank.hip), each against a plain float64
restatement of its operation (tests/ref64.py, pinned on the CPU by tests/test_ref64.py) at the shapes where such kernels go wrong:
lane tails (T < 64, T = 64 k +- 1), row tails (R % 4 != 0), strided views, grid limits, exact ties and NaN conventions.
Needs a real MI355X: run with `-m gpu` (`-s` prints, per kernel, the largest ratio of observed error to the bound).

ERROR BOUNDS are derived, not tuned.  U = 2^-24 is the unit roundoff of float32.  A sum of n terms on one wave collects
k(n) = ceil(n / 64) + 8 roundings (one per sequential add of a lane, six shuffle levels, the multiply / divide around it), so its error
is at most k(n) U S with S = sum |term| from ref64; each test propagates that to first order (or, for square roots near a clamp, through
the interval) to the kernel's output, in the test itself.  Copies and selections must be torch.equal to the float32 CPU result.  Math functions
get the maximum ULP error the HIP programming guide tabulates ("HIP math API", single-precision mathematical functions): expf 1, logf 2,
tanhf 2, sincospif 1 ULP (1 ULP = 2 U relative); division and sqrtf are correctly rounded in this build (no fast-math flags: U each).
A ratio above 1 fails.

MEASURED on an MI355X (profiles/small_kernels_error_ratios.txt), largest error / bound per kernel:
  melspec_logmel 0.34 (unit impulse, n = 513) | instnorm_rows 0.25 | row_mean 0.24 | l2norm_rows 0.42 | se_gate_add 0.99 | tanh_inplace 0.52
  attentive_stats mean 0.18, std 0.92 (one-hot logits: the variance cancels to the clamp) | f0_stats mean 0.026, std 0.035 | f0_apply 0.037
  f0_mean_reversion 0.35 | log_softmax_channels 0.53 | add3, assemble_input, pad_replicate, quantise + noise: equal bit for bit.
A bound of one rounding (the last add of se_gate_add) is met to 0.99 by some element among thousands, as a half-ULP bound must be; the F0
statistics sit lowest because their 1024-thread block sums far fewer terms per thread than the count of roundings allows for.
FINDINGS.  (1) attentive_stats' variance m2 - m1^2 (the reference's formula) cancels: for rows of mean 50 and deviation 0.1 the derived bound
on the std is as wide as the std itself, so that case can only check the mean and the clamp.  (2) The device's logf(1e-6f) is 1 ULP below
the correctly rounded value (inside the documented 2).  (3) This HIP runtime accepts grids beyond 65535 blocks in y and z: pad_replicate at
B C = 65536 and 131072 and assemble_input at B = 65536 launched and were right before the row loop and the size checks existed.
The file's 544 cases take 5 s on the GPU; the whole -m gpu suite with them, 1023 tests, takes 137 s (the parent commit's 479: 132 s).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref64
from ref64 import U

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 * U                   # relative size of one unit in the last place, at worst
EXP_ULP, LOG_ULP, TANH_ULP = 1, 2, 2          # HIP programming guide, "HIP math API": maximum ULP error of expf / logf / tanhf
TINY = 2.0 ** -126              # results below the smallest normal float32 may be flushed or denormal: an absolute allowance

T_GRID = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 4099)
R_GRID = (1, 3, 4, 5, 1027)
KINDS = ("randn", "mean100_std0.01", "constant")

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    """prints the largest error / bound ratio of every kernel when the module is done (and writes the table to the file
    SAT_SMALL_KERNEL_RATIOS names, if set)"""
    yield
    lines = [f"{k:28s} {r:8.4f}   at {case}" for k, (r, case) in sorted(_RATIOS.items())]
    print("\nlargest observed error / derived bound, per kernel:\n" + "\n".join(lines))
    path = os.environ.get("SAT_SMALL_KERNEL_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_small_kernels.py: largest observed error / derived bound, per kernel (a ratio above 1 fails)\n")
            f.write("\n".join(lines) + "\n")


def _ops():
    import satools_amd  # noqa: F401
    from satools_amd import ops
    return ops


def _lib():
    import satools_amd  # noqa: F401
    from satools_amd import _lib
    return _lib


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _check(kernel, case, got, want, bound):
    """got (device or CPU float32) against want (float64) within `bound` (float64, elementwise, broadcastable); a bound of 0 demands
    equality.  Records and prints the largest err / bound."""
    got = got.detach().cpu().double()
    want = want.double()
    assert got.shape == want.shape, (kernel, case, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), (kernel, case, "non-finite output")
    err = (got - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = float(ratio.max())
    print(f"{kernel} [{case}]: max error {float(err.max()):.3e}, max error / bound {r:.4f}")
    if r > _RATIOS.get(kernel, (-1.0, ""))[0]:
        _RATIOS[kernel] = (r, case)
    assert r <= 1.0, (kernel, case, r, float(err.max()))
    return r


def _rows(kind, R, T, g):
    if kind == "randn":
        return torch.randn(R, T, generator=g)
    if kind == "mean100_std0.01":
        return (100.0 + 0.01 * torch.randn(R, T, generator=g)).float()
    return (torch.randn(R, 1, generator=g) * 10).expand(R, T).contiguous()


def _still_works():
    """after a refused call: a small valid one runs and is right (no sticky device error was left behind)"""
    x = torch.tensor([[3.0, 4.0], [0.0, 0.0], [-6.0, 8.0]])
    y = _ops().l2norm_rows(x.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.tensor([[0.6, 0.8], [0.0, 0.0], [-0.6, 0.8]]))


# ---- melspec_logmel --------------------------------------------------------------------------------------------------
FFT_ROUNDINGS = 84      # |dX_k| <= 84 U A, A = sum |windowed sample|: 10 radix-2 stages x (complex multiply 3 U + twiddle from sincospif
                        # 1 ULP per component ~ 4 U + add 1 U) + pre-emphasis and window (multiply, subtract, multiply: 3 U), rounded up


def _front_end_consts():
    from satools_amd import xvector
    return torch.hann_window(400, periodic=True), xvector.mel_filterbank().t().contiguous()      # [400], [80, 513]


def _signal(kind, B, n, g):
    if kind == "noise":
        return torch.randn(B, n, generator=g) * 0.3
    if kind == "dc0.5":
        return torch.full((B, n), 0.5)
    x = torch.zeros(B, n)
    if kind == "impulse_first":
        x[:, 0] = 1.0
    elif kind == "impulse_last":
        x[:, n - 1] = 1.0
    if B > 1 and kind != "zeros":
        x[1] *= -0.5                       # rows differ: a kernel that read row 0 for every utterance would be seen
    return x


@pytest.mark.parametrize("B", (1, 3), ids=lambda b: f"B{b}")
@pytest.mark.parametrize("n", (513, 640, 799, 800, 801, 16000, 24123), ids=lambda n: f"n{n}")
@pytest.mark.parametrize("kind", ("noise", "dc0.5", "zeros", "impulse_first", "impulse_last"))
def test_melspec_logmel(kind, n, B):
    ops = _ops()
    window, fb = _front_end_consts()
    wav = _signal(kind, B, n, _gen(1, n, B))
    out = ops.melspec_logmel(wav.to(DEV), window.to(DEV), fb.to(DEV), 0.97).cpu()
    assert out.shape == (B, 80, 1 + n // 160)
    if kind == "zeros":
        # every mel power is exactly 0, so every output is the device's logf(1e-6f): one value everywhere, no FFT residue.  That value is
        # the device's own logf (torch.log on the device), LOG_ULP ULPs at most from the correctly rounded one (measured: 1 ULP below it)
        floor = float(torch.log(torch.tensor(1e-6, dtype=torch.float32, device=DEV)).cpu())
        exact = math.log(float(np.float32(1e-6)))
        assert abs(floor - exact) <= LOG_ULP * ULP * abs(exact), (floor, exact)
        assert bool((out == floor).all()), (float(out.min()), float(out.max()), floor)
        return
    mel, aux = ref64.melspec(wav, window, fb, 0.97)
    dX = FFT_ROUNDINGS * U * aux["A"].unsqueeze(2)                               # [B, frames, 1]
    dP = 2 * aux["amp"] * dX + dX * dX + 3 * U * aux["power"]                    # re^2 + im^2: two squares and an add
    taps = (fb > 0).sum(1).double().view(1, -1, 1)                               # the FMA chain over a filter's taps: one rounding each
    dM = torch.matmul(dP, fb.double().t()).transpose(1, 2) + (taps + 1) * U * mel
    c = ref64.f32(1e-6)
    # compared in the power domain (near the 1e-6 floor the log turns a tiny absolute error into a large one): exp(out) against
    # mel + 1e-6, with the rounding of that add (U) and logf's LOG_ULP ULPs of |out| carried through the exponential
    lg = torch.log(mel + c)
    bound = dM + (mel + c) * (U + LOG_ULP * ULP * lg.abs())
    _check("melspec_logmel", f"{kind}-n{n}-B{B}", torch.exp(out.double()), mel + c, bound)


def test_melspec_logmel_refuses_an_utterance_shorter_than_the_padding():
    ops, SatError = _ops(), _lib().SatError
    window, fb = _front_end_consts()
    with pytest.raises(SatError, match="shorter than the reflect padding"):
        ops.melspec_logmel(torch.zeros(1, 512, device=DEV), window.to(DEV), fb.to(DEV), 0.97)
    _still_works()


# ---- one wave per row: instnorm, row_mean, l2norm ------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID, ids=lambda t: f"T{t}")
@pytest.mark.parametrize("R", R_GRID, ids=lambda r: f"R{r}")
def test_instnorm_rows(R, T):
    ops = _ops()
    k = ref64.reduction_terms(T)
    eps = 1e-5
    for kind in KINDS:
        x = _rows(kind, R, T, _gen(2, R, T, len(kind)))
        got = ops.instnorm_rows(x.view(1, R, T).to(DEV), eps)[0]
        want, a = ref64.instance_norm(x, eps)
        d = x.double() - a["mean"]
        dmean = k * U * a["S1"] / T                                              # the sum, then / T (inside the +8)
        dd = dmean + U * d.abs()                                                 # x - mean
        # sum d^2: its own roundings (k), each d's rounding (2 U d^2), and the error e of the mean, common to the row: sum (d + e)^2 =
        # sum d^2 + 2 e sum d + T e^2 with sum d = 0 exactly, so e enters squared (and through the rounding of d, to second order)
        dq = (k + 2) * U * a["S2"] + T * dmean ** 2 + 2 * dmean * U * d.abs().sum(-1, keepdim=True)
        v = a["var"] + ref64.f32(eps)
        dv = dq / T + U * a["var"] + U * v                                       # / T, + eps
        rstd = 1.0 / torch.sqrt(v)
        drstd = torch.maximum(1.0 / torch.sqrt((v - dv).clamp(min=1e-300)) - rstd, rstd - 1.0 / torch.sqrt(v + dv)) + 2 * U * rstd     # sqrt, 1 / .
        bound = dd * (rstd + drstd) + d.abs() * drstd + U * want.abs()           # a constant row: d = 0, the bound is dmean * rstd around 0
        _check("instnorm_rows", f"{kind}-R{R}-T{T}", got, want, bound)


@pytest.mark.parametrize("T", T_GRID, ids=lambda t: f"T{t}")
@pytest.mark.parametrize("R", R_GRID, ids=lambda r: f"R{r}")
def test_row_mean(R, T):
    ops = _ops()
    k = ref64.reduction_terms(T)
    for kind in KINDS:
        x = _rows(kind, R, T, _gen(3, R, T, len(kind)))
        got = ops.row_mean(x.view(1, R, T).to(DEV))
        assert got.shape == (1, R, 1)
        want, a = ref64.row_mean(x)
        _check("row_mean", f"{kind}-R{R}-T{T}", got[0], want, k * U * a["S1"] / T)


@pytest.mark.parametrize("D", T_GRID, ids=lambda t: f"D{t}")
@pytest.mark.parametrize("R", R_GRID, ids=lambda r: f"R{r}")
def test_l2norm_rows(R, D):
    ops = _ops()
    k = ref64.reduction_terms(D)
    for kind in KINDS + ("zero_rows",):
        x = _rows("randn" if kind == "zero_rows" else kind, R, D, _gen(4, R, D, len(kind)))
        if kind == "zero_rows":
            x[::2] = 0.0                                                         # an all-zero row: zeros (the 1e-12 floor), not NaN
        got = ops.l2norm_rows(x.to(DEV))
        want, a = ref64.l2norm(x)
        nrm = a["nrm"].clamp(min=1e-300)
        dn = k * U * a["S"] / (2 * nrm) + U * nrm                                # sum x^2, sqrt
        bound = want.abs() * (dn / nrm + U)                                      # x / nrm
        _check("l2norm_rows", f"{kind}-R{R}-D{D}", got, want, bound)
        if kind == "zero_rows":
            assert not got.cpu()[::2].any()


# ---- add3, se_gate_add, tanh -----------------------------------------------------------------------------------------
def _slice_of(B, ctot, c0, C, T, pitch, g, poison=None):
    """a [B, C, T] view into a [B, ctot, pitch] buffer: channel slice c0 .. c0 + C, the first T of `pitch` columns"""
    buf = torch.randn(B, ctot, pitch, generator=g) if poison is None else torch.full((B, ctot, pitch), poison)
    return buf, (slice(None), slice(c0, c0 + C), slice(0, T))


@pytest.mark.parametrize("with_c", (False, True), ids=("a+b", "a+b+c"))
@pytest.mark.parametrize("B,C,T", [(1, 1, 1), (2, 3, 63), (1, 5, 64), (2, 4, 65), (33, 3, 129), (2, 5, 255), (1, 3, 256), (2, 1, 257), (2, 3, 1000),
                                   (1, 2, 4099)], ids=lambda v: str(v))
def test_add3_on_channel_slices(B, C, T, with_c):
    ops = _ops()
    g = _gen(5, B, C, T, with_c)
    POISON = -12345.0
    # the way xvector.py calls it: channel slices of wider tensors (batch stride != C * T), here also with a row pitch (channel stride != T)
    for pitch in (T, T + 3):
        abuf, asl = _slice_of(B, 2 * C + 1, 1, C, T, pitch, g)
        bbuf, bsl = _slice_of(B, C + 2, 2, C, T, pitch, g)
        cbuf, csl = _slice_of(B, 3 * C, C, C, T, pitch, g)
        ybuf, ysl = _slice_of(B, 3 * C + 1, 2 * C, C, T, pitch, g, poison=POISON)
        want = abuf[asl] + bbuf[bsl]
        if with_c:
            want = want + cbuf[csl]                                              # left to right, like out1 + out2 + out3
        yd = ybuf.to(DEV)
        ad, bd, cd = abuf.to(DEV), bbuf.to(DEV), cbuf.to(DEV)
        ret = ops.add3(ad[asl], bd[bsl], cd[csl] if with_c else None, out=yd[ysl])
        assert ret.data_ptr() == yd[ysl].data_ptr()
        got = yd.cpu()
        assert torch.equal(got[ysl], want), (B, C, T, pitch, float((got[ysl] - want).abs().max()))
        mask = torch.ones_like(got, dtype=torch.bool)
        mask[ysl] = False
        assert bool((got[mask] == POISON).all()), "add3 wrote outside its slice"
        # and into a fresh contiguous output
        assert torch.equal(ops.add3(ad[asl], bd[bsl], cd[csl] if with_c else None).cpu(), want)
    _RATIOS.setdefault("add3", (0.0, "torch.equal to the float32 CPU sum in every case"))


GATE_LOGITS = (-100.0, -20.0, 0.0, 20.0, 100.0)


@pytest.mark.parametrize("n_skips", (0, 1, 2, 3), ids=lambda s: f"skips{s}")
@pytest.mark.parametrize("B,C,T", [(1, 1, 1), (2, 5, 63), (1, 7, 64), (2, 5, 65), (33, 5, 129), (1, 6, 256), (2, 5, 257), (1, 5, 4099)], ids=lambda v: str(v))
def test_se_gate_add(B, C, T, n_skips):
    ops = _ops()
    g = _gen(6, B, C, T, n_skips)
    POISON = -12345.0
    z = torch.randn(B, C, T, generator=g)
    logits = torch.tensor([GATE_LOGITS[(b + c) % 5] for b in range(B) for c in range(C)]).view(B, C)
    logits = torch.where(torch.rand(B, C, generator=g) < 0.3, torch.randn(B, C, generator=g) * 3, logits)
    skips = [torch.randn(B, C, T, generator=g) for _ in range(n_skips)]
    want, a = ref64.se_gate_add(z, logits, skips)
    # gate = 1 / (1 + expf(-g)): expf EXP_ULP ULPs on e, damped by e / (1 + e) <= 1; the add and the divide U each.  Then z * gate (U) and one
    # rounding per skip add, each of its own partial sum.  TINY |z|: sigmoid(-100) = 3.7e-44 is below the normal range (expf(100) = inf -> 0)
    bound = a["prod"] * (EXP_ULP * ULP + 2 * U + U) + U * a["partials"] + TINY * z.double().abs()
    ybuf = torch.full((B, 2 * C + 3, T), POISON)
    ysl = (slice(None), slice(C + 1, 2 * C + 1), slice(None))                    # the `cat[:, C:2C]` slice of xvector.py
    yd = ybuf.to(DEV)
    ops.se_gate_add(z.to(DEV), logits.view(B, C, 1).to(DEV), [s.to(DEV) for s in skips], out=yd[ysl])
    got = yd.cpu()
    _check("se_gate_add", f"B{B}-C{C}-T{T}-skips{n_skips}", got[ysl], want, bound)
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[ysl] = False
    assert bool((got[mask] == POISON).all()), "se_gate_add wrote outside its slice"
    if n_skips == 0:
        half = (logits == 0.0).view(B, C, 1).expand_as(z)
        assert torch.equal(got[ysl][half], (z * 0.5)[half])                      # sigmoid(0) = 1/2 exactly


@pytest.mark.parametrize("n", (1, 63, 255, 256, 257, 4099, 3 * 4099), ids=lambda n: f"n{n}")
def test_tanh_inplace(n):
    ops = _ops()
    x = torch.randn(n, generator=_gen(7, n)) * 3
    special = torch.tensor([0.0, -0.0, 1e-8, -1e-8, 1e-3, 0.5, -0.5, 9.0, -9.0, 20.0, -20.0, 100.0, -100.0])
    x[:min(n, special.numel())] = special[:n]
    xd = x.to(DEV)
    assert ops.tanh_(xd).data_ptr() == xd.data_ptr()
    want = ref64.tanh(x)
    _check("tanh_inplace", f"n{n}", xd, want, TANH_ULP * ULP * want.abs() + 2.0 ** -149)


# ---- attentive_stats -------------------------------------------------------------------------------------------------
def _attentive_bounds(a, mean, std, T):
    k = ref64.reduction_terms(T)
    # e_t = expf(l_t - max): the subtraction rounds the argument by U |l_t - max|, expf adds EXP_ULP ULPs; sum e: k U and the terms' own errors
    rho = (k + a["Ew"] + EXP_ULP * 2) * U                                        # relative error of sum_t e_t
    wfix = (EXP_ULP * 2 + 1) * U + rho                                           # of w_t = e_t / se, without its U (max - l_t) part (in E1 / E2)
    dm1 = k * U * a["S1"] + U * a["E1"] + wfix * a["S1"]
    dm2 = (k + 1) * U * a["S2"] + U * a["E2"] + wfix * a["S2"]
    dvar = dm2 + 2 * mean.abs() * dm1 + dm1 ** 2 + U * mean ** 2 + U * a["var"].abs()           # m2 - m1 * m1
    c = ref64.f32(1e-9)
    lo, hi = torch.sqrt((a["var"] - dvar).clamp(min=c)), torch.sqrt((a["var"] + dvar).clamp(min=c))
    # = dvar / (2 std) to first order; the interval form stays right where var - dvar reaches the 1e-9 clamp
    dstd = torch.maximum(std - lo, hi - std) + U * hi
    return dm1, dstd


@pytest.mark.parametrize("B,C,T", [(1, 1, 1), (1, 3, 2), (2, 5, 63), (1, 4, 64), (2, 3, 65), (1, 5, 127), (33, 1, 128), (2, 2, 129), (1, 1027, 37),
                                   (2, 3, 1000), (1, 5, 4099), (33, 3, 65)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ("random", "mean50_std0.1", "one_hot_80", "uniform_logits", "x_zero"))
def test_attentive_stats(kind, B, C, T):
    ops = _ops()
    g = _gen(8, B, C, T, len(kind))
    x = torch.randn(B, C, T, generator=g)
    logits = torch.randn(B, C, T, generator=g) * 2
    if kind == "mean50_std0.1":
        x = (50.0 + 0.1 * x).float()
    elif kind == "one_hot_80":
        logits.scatter_(2, torch.randint(0, T, (B, C, 1), generator=g), 80.0)
    elif kind == "uniform_logits":
        logits = torch.full((B, C, T), 1.25)
    elif kind == "x_zero":
        x = torch.zeros(B, C, T)
    out = ops.attentive_stats(x.to(DEV), logits.to(DEV)).cpu()
    assert out.shape == (B, 2 * C, 1)
    gm, gs = out[:, :C, 0], out[:, C:, 0]
    mean, std, a = ref64.attentive_stats(x, logits)
    if kind == "x_zero":
        assert not gm.any() and bool((gs == float(np.sqrt(np.float32(1e-9)))).all())           # exactly sqrtf(1e-9f)
        return
    dm1, dstd = _attentive_bounds(a, mean, std, T)
    _check("attentive_stats.mean", f"{kind}-B{B}-C{C}-T{T}", gm, mean, dm1)
    _check("attentive_stats.std", f"{kind}-B{B}-C{C}-T{T}", gs, std, dstd)
    if T == 1:
        assert torch.equal(gm, x[:, :, 0])                                       # the one weight is exactly 1


# ---- F0: statistics, normalisation, quantisation, noise ----------------------------------------------------------------
def _f0_track(n, g, voiced=0.6):
    f0 = 80.0 + 220.0 * torch.rand(n, generator=g)
    return torch.where(torch.rand(n, generator=g) < voiced, f0, torch.zeros(n))


def _f0_stats_gpu(f0d):
    l = _lib()
    stats = torch.empty(2, dtype=torch.float32, device=DEV)
    l.check(l.lib().sat_f0_stats_f32(l.ptr(f0d), f0d.numel(), l.ptr(stats), l.stream()), "sat_f0_stats_f32")
    return stats.cpu()


@pytest.mark.parametrize("n", (1, 63, 1023, 1024, 1025, 8007), ids=lambda n: f"n{n}")
def test_f0_stats_and_normalisation(n):
    ops = _ops()
    f0 = _f0_track(n, _gen(9, n))
    f0[0] = 123.0                                                                # n = 1: the one voiced value, a NaN std
    if n > 1:
        f0[n - 1] = 0.0                                                          # a voiced and an unvoiced value at the ends
    want, a = ref64.f0_normalise(f0)
    cnt = a["count"]
    stats = _f0_stats_gpu(f0.to(DEV))
    got = ops.f0_norm_transform_(f0.to(DEV).clone())
    if cnt < 2:                                                                  # torch: var of one value is NaN (and the mean of none)
        assert math.isnan(float(stats[1])) and (cnt == 1 or math.isnan(float(stats[0])))
        assert bool(torch.isnan(got.cpu()[f0 != 0]).all()) and not got.cpu()[f0 == 0].any()
        return
    # a block of 1024 threads: ceil(n / 1024) adds per thread, six shuffle levels, 16 wave partials added in turn, the divide
    k = math.ceil(n / 1024) + 6 + 16 + 2
    d = torch.where(f0 != 0, f0.double() - a["mean"], torch.zeros(n, dtype=torch.float64))
    dmean = k * U * a["S1"] / cnt
    dd = dmean + U * d.abs()
    dS = (k + 2) * U * a["S2"] + cnt * dmean ** 2 + 2 * dmean * U * d.abs().sum()          # (the mean's error enters squared: sum d = 0, as in instnorm)
    v = a["var"] + ref64.f32(1e-6)
    dv = dS / (cnt - 1) + U * a["var"] + U * v
    dstd = dv / (2 * a["std"]) + U * a["std"]                                    # dv << v for these tracks (a spread of tens of Hz)
    assert float(dv / v) < 1e-3
    _check("f0_stats.mean", f"n{n}", stats[0], a["mean"], dmean)
    _check("f0_stats.std", f"n{n}", stats[1], a["std"], dstd)
    bound = dd / a["std"] + want.abs() * (dstd / a["std"] + U)
    _check("f0_apply.normalise", f"n{n}", got, want, bound)
    assert not got.cpu()[f0 == 0].any()
    # quantisation and noise act on the normalised float32 values: exact functions of them (x * bins, round half to even, / bins for a power
    # of two; one addition), so the expected result is torch's on the kernel's own normalised track, bit for bit
    norm = got.cpu()
    for bins in (16, 64):
        q = torch.where(norm != 0, torch.round(norm * bins) / bins, torch.zeros(n))
        gq = ops.f0_norm_transform_(f0.to(DEV).clone(), quant_bins=bins).cpu()
        assert torch.equal(gq, q), (n, bins)
        noise = torch.randn(n, generator=_gen(10, n, bins))
        gn = ops.f0_norm_transform_(f0.to(DEV).clone(), quant_bins=bins, noise=noise.to(DEV)).cpu()
        assert torch.equal(gn, torch.where(q != 0, q + noise, torch.zeros(n))), (n, bins)
    _RATIOS.setdefault("f0_apply.quantise+noise", (0.0, "torch.equal to torch.round / the float32 sum in every case"))


def test_f0_all_unvoiced_gives_a_nan_mean_like_torch():
    f0 = torch.zeros(100)
    stats = _f0_stats_gpu(f0.to(DEV))
    assert math.isnan(float(stats[0])) and math.isnan(float(torch.zeros(0).mean()))
    assert not _ops().f0_norm_transform_(f0.to(DEV)).cpu().any()                 # and every zero stays zero
    _still_works()


def _f0_apply_gpu(x, stats, bins, noise=None):
    l = _lib()
    xd, sd = x.to(DEV).clone(), torch.tensor(stats, dtype=torch.float32, device=DEV)
    nd = noise.to(DEV) if noise is not None else None
    l.check(l.lib().sat_f0_apply_f32(l.ptr(xd), xd.numel(), l.ptr(sd), int(bins), l.ptr(nd), l.stream()), "sat_f0_apply_f32")
    return xd.cpu()


@pytest.mark.parametrize("bins", (1, 16, 64), ids=lambda b: f"bins{b}")
def test_f0_apply_rounds_exact_ties_to_even(bins):
    """stats = [0, 1] make the normalisation the identity, (k + 0.5) / bins is exact in float32: every input is an exact tie"""
    kk = torch.arange(-3 * bins - 2, 3 * bins + 3, dtype=torch.float32)
    x = (kk + 0.5) / bins
    assert torch.equal(x * bins, kk + 0.5)
    want = torch.round(x * bins) / bins                                          # torch.round: half to even
    assert not torch.equal(want, torch.floor(x * bins + 0.5) / bins)             # (half up would differ)
    got = _f0_apply_gpu(x, [0.0, 1.0], bins)
    assert torch.equal(got, want), (got[got != want][:8], want[got != want][:8])


def test_f0_apply_keeps_a_value_quantised_to_zero_at_zero_under_noise():
    x = torch.tensor([0.01, -0.02, 0.03124, 0.0, 0.04, 1.0, -0.031])            # x * 16 in (-0.5, 0.5) -> 0, except 0.04 and 1.0
    noise = torch.tensor([0.7, -0.3, 0.2, 0.9, 0.5, -0.25, 0.4])
    got = _f0_apply_gpu(x, [0.0, 1.0], 16, noise)
    q = torch.round(x * 16) / 16
    assert q.tolist() == [0.0, -0.0, 0.0, 0.0, 0.0625, 1.0, -0.0]
    assert torch.equal(got, torch.where(q != 0, q + noise, torch.zeros(7)))
    assert got.tolist()[:4] == [0.0, 0.0, 0.0, 0.0] and got.tolist()[6] == 0.0
    # without quantisation the noise lands on every non-zero value
    assert torch.equal(_f0_apply_gpu(x, [0.0, 1.0], 0, noise), torch.where(x != 0, x + noise, torch.zeros(7)))


# ---- f0_mean_reversion -----------------------------------------------------------------------------------------------
def _mean_reversion_gpu(x, alpha, n):
    l = _lib()
    xd = x.to(DEV).contiguous()
    out = torch.empty_like(xd)
    l.check(l.lib().sat_f0_mean_reversion_f32(l.ptr(xd), l.ptr(out), xd.shape[-1], C.c_float(alpha), int(n), l.stream()), "sat_f0_mean_reversion_f32")
    return out.cpu()


@pytest.mark.parametrize("alpha", (0.0, 0.5, 1.0), ids=lambda a: f"alpha{a}")
@pytest.mark.parametrize("n", (1, 2, 32, 33), ids=lambda n: f"n{n}")
@pytest.mark.parametrize("T", (1, 5, 31, 32, 33, 300), ids=lambda t: f"T{t}")
def test_f0_mean_reversion(T, n, alpha):
    from oracle import f0 as of0
    g = _gen(11, T, n)
    x = torch.randn(1, 1, T, generator=g) * (torch.rand(1, 1, T, generator=g) > 0.3)          # a normalised track: O(1), zeros where unvoiced
    got = _mean_reversion_gpu(x, alpha, n)
    # the CPU oracle (torch's conv1d), with the bar of test_hip_yaapt.py::test_mean_reversion_option_matches_golden: bit for bit for the
    # short windows, one ulp of O(1) values (2.4e-7) from 32 taps on, where torch's conv1d sums in an order of its own
    ref = of0.mean_reversion(x.clone(), alpha, n)
    err = float((got - ref).abs().max())
    print(f"f0_mean_reversion [T{T}-n{n}-alpha{alpha}]: max |kernel - CPU oracle| = {err:.3e}")
    if n >= 32:
        assert err <= 2.4e-7, (T, n, alpha, err)
    else:
        assert np.array_equal(got.numpy(), ref.numpy()), (T, n, alpha, err)
    # float64: an FMA chain of n taps (one rounding each, and w x_0), alpha * avg, (1 - alpha) * x, their sum
    want, a = ref64.mean_reversion(x, alpha, n)
    bound = a["alpha"] * (n + 1) * U * a["S"] + U * ((a["one_minus_alpha"] * x.double()).abs() + (a["alpha"] * a["avg"]).abs()) + U * want.abs()
    _check("f0_mean_reversion", f"T{T}-n{n}-alpha{alpha}", got, want, bound)


# ---- assemble_input --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 5), ids=lambda b: f"B{b}")
@pytest.mark.parametrize("n_spk", (0, 1, 247), ids=lambda s: f"spk{s}")
@pytest.mark.parametrize("T_f0,T", [(250, 250), (251, 250), (249, 250), (3, 7), (7, 3), (1, 9), (500, 4099)], ids=lambda v: str(v))
def test_assemble_input(T_f0, T, n_spk, B):
    ops = _ops()
    g = _gen(12, T_f0, T, n_spk, B)
    for c_bn in (1, 3, 48):
        bn = torch.randn(B, c_bn, T, generator=g)
        f0 = torch.randn(B, 1, T_f0, generator=g)
        spk = torch.randn(B, n_spk, generator=g) if n_spk else None
        got = ops.assemble_input(bn.to(DEV), f0.to(DEV), spk.to(DEV) if n_spk else None, n_spk)
        want = ref64.assemble_input(bn, f0, spk)
        assert got.shape == (B, c_bn + 1 + n_spk, T)
        assert torch.equal(got.cpu(), want), (c_bn, int((got.cpu() != want).sum()))
    _RATIOS.setdefault("assemble_input", (0.0, "torch.equal to cat(bn, F.interpolate(f0, nearest), spk) in every case"))


def test_oversize_batches_are_refused_with_a_message():
    """B (and the channel count) are grid dimensions of assemble_input and tdnnf_unfold15: beyond 65535 the call names the limit instead
    of failing to launch; the host API refuses it, nothing reaches the device"""
    ops, SatError = _ops(), _lib().SatError
    B = 65536
    with pytest.raises(SatError, match="assemble_input: batch of 65536"):
        ops.assemble_input(torch.zeros(B, 1, 1, device=DEV), torch.zeros(B, 1, 1, device=DEV), None, 0)
    _still_works()
    with pytest.raises(SatError, match="assemble_input: 65536 channels"):
        ops.assemble_input(torch.zeros(1, 65535, 1, device=DEV), torch.zeros(1, 1, 1, device=DEV), None, 0)
    g = _gen(13)
    bn, f0 = torch.randn(2, 3, 7, generator=g), torch.randn(2, 1, 4, generator=g)
    assert torch.equal(ops.assemble_input(bn.to(DEV), f0.to(DEV), None, 0).cpu(), ref64.assemble_input(bn, f0, None))
    with pytest.raises(SatError, match="tdnnf_unfold15: batch of 65536"):
        ops.tdnnf_unfold15(torch.zeros(B, 2, 2, device=DEV))
    _still_works()
    for D, T in ((4, 1), (4, 2), (6, 7), (16, 40)):
        x = torch.randn(3, D, T, generator=g)
        win, byp = ops.tdnnf_unfold15(x.to(DEV))
        rw, rb = ref64.tdnnf_unfold15(x)
        assert torch.equal(win.cpu(), rw) and torch.equal(byp.cpu(), rb), (D, T)


# ---- pad_replicate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleave", (False, True), ids=("replicate", "interleave_right"))
@pytest.mark.parametrize("right", (0, 4, 19), ids=lambda r: f"right{r}")
@pytest.mark.parametrize("left", (0, 4, 19), ids=lambda l: f"left{l}")
def test_pad_replicate(left, right, interleave):
    ops = _ops()
    g = _gen(14, left, right, interleave)
    for B, c, T in ((1, 1, 1), (3, 5, 1), (2, 3, 5), (5, 4, 300), (33, 2, 255), (4, 3, 250)):
        x = torch.randn(B, c, T, generator=g)
        got = ops.pad_replicate(x.to(DEV), left, right, interleave_right=interleave).cpu()
        want = ref64.pad_replicate(x, left, right, interleave)
        assert got.shape == (B, c, left + T + right)
        assert torch.equal(got, want), (B, c, T, int((got != want).sum()))
        if not interleave:
            assert torch.equal(want, F.pad(x, (left, right), mode="replicate"))
        elif right:                                                              # the definition in fbank.hip: utterance (b * right + p) mod B
            for b in range(B):
                for p in (0, right - 1):
                    assert torch.equal(got[b, :, left + T + p], x[(b * right + p) % B, :, T - 1])
    _RATIOS.setdefault("pad_replicate", (0.0, "torch.equal to F.pad(mode='replicate') / the pad_input definition in every case"))


@pytest.mark.parametrize("interleave", (False, True), ids=("replicate", "interleave_right"))
@pytest.mark.parametrize("B,c", [(1, 65535), (64, 1024), (128, 1024), (65536, 1), (3, 43691)], ids=lambda v: str(v))
def test_pad_replicate_beyond_the_grid_limit(B, c, interleave):
    """B * C rows: 65535 fits the y dimension of a grid, 65536 (the wav2vec2 ASR forward at batch 64 x 1024 channels) and more do not"""
    ops = _ops()
    x = torch.randn(B, c, 3, generator=_gen(15, B, c))
    got = ops.pad_replicate(x.to(DEV), 4, 4, interleave_right=interleave).cpu()
    assert torch.equal(got, ref64.pad_replicate(x, 4, 4, interleave))
    got = ops.pad_replicate(x[:, :, :1].contiguous().to(DEV), 0, 1, interleave_right=interleave).cpu()
    assert torch.equal(got, ref64.pad_replicate(x[:, :, :1], 0, 1, interleave))


# ---- log_softmax_channels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (4.0, 60.0), ids=lambda s: f"x{s:g}")
@pytest.mark.parametrize("T", (1, 15, 16, 17, 37), ids=lambda t: f"T{t}")
@pytest.mark.parametrize("Cn", (1, 5, 16, 17, 3280), ids=lambda c: f"C{c}")
def test_log_softmax_channels(Cn, T, scale):
    ops = _ops()
    for B in (1, 3):
        x = torch.randn(B, Cn, T, generator=_gen(16, Cn, T, B)) * scale          # x 60: a plain exp(x) overflows float32
        if scale > 50 and x.numel() >= 1000:
            assert not bool(torch.isfinite(torch.exp(x)).all())
        xd = x.to(DEV)
        assert ops.log_softmax_channels_(xd).data_ptr() == xd.data_ptr()
        want, a = ref64.log_softmax_channels(x)
        lse = a["lse"]
        groups = math.ceil(Cn / 16)
        # the sums: (C / 16 + 24) U max(1, |lse|).  expf: an argument x - max rounded by U |x - max| (the running rescales telescope to the
        # same total) and EXP_ULP ULPs per factor, at most one rescale per channel of a lane and the merge: weighted by the softmax itself.
        # logf: LOG_ULP ULPs of |log tot|.  Then x - lse rounds once
        dlse = (Cn / 16 + 24) * U * lse.abs().clamp(min=1.0) + U * (a["E"] + EXP_ULP * 2 * (groups + 2)) + LOG_ULP * ULP * a["logtot"].abs()
        _check("log_softmax_channels", f"C{Cn}-T{T}-x{scale:g}-B{B}", xd, want, dlse + U * want.abs())
