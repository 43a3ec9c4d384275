"""The packed real-input FFT of csrc/yaapt.hip (fft_load_packed, fft_pass / fft_from, fft_packed_mag), restated in float32 numpy
operation by operation and judged on the CPU by the running float64 bound of tests/ref64_yaapt.fft_running.  CPU only: the check to
run before any time is spent on the device.

Restated exactly as the kernels do it:
  * the load: thread -> (lane, wave), lane -> (r, q), point m = (q << 6) | (wave * ROUNDS + round), samples 2m and 2m + 1 (zero past
    the frame: an odd frame's last imaginary part) to re / im[brev12(m) + r]; z = 3, 2, 1, 0 leading copy stages by the packed
    length Lp = ceil(L / 2) <= 512, 1024, 2048, more;
  * stages z + 1 .. 12, radix-2 decimation in time, twiddle = entry (h - 1) + p of the staged table built from the host's float32
    table exp(-2 pi i k / 8192), four-multiply complex product, no fused operation (the library is built with -ffp-contract=off);
    the kernel's grouping of stages into passes changes no operation and is not restated;
  * the untangle of a wanted bin k from Z[k] and Z[4096 - k], k = 0 in its own form, halving by an exact multiply.
The restatement also proves what the load's comment claims: every element of re and im is written exactly once (nothing is zero
filled), and the 32 lanes of each half of a wave store to 32 distinct banks (a 4-byte store is banked modulo 32 per half wave).

Inputs: the float32 windowed frames of the catalogue of tests/yaapt_cases.py as the kernels form them (hann product; kaiser product
minus the float32 mean), taken AS GIVEN: they enter fft_running exactly, with no input error, so the bound is the transform's own and
tighter than what the device test grants the same bins.  Rounding counts: cmul = 3.25 as in tests/test_hip_yaapt_stages.py (table
twiddle 1 U + four-multiply product sqrt 5 U).  The untangle adds no count of its own: E and O take one rounding each, as the sum
a + wb of a stage does; the halving is exact."""
import numpy as np
import pytest
import torch

import ref64_yaapt as r64
import yaapt_cases as yc
from oracle import biquad
from oracle import yaapt as oy

LOG, N, T = 12, 4096, 512
R = r64.Roundings(cmul=3.25, hyp=4, nl_sum=None, en_mean=None, sp_mean=None, shc_sum=None, shc_avg=None, fm_head=None, fm_tail=None,
                  dot=None, pw=None)
f32 = np.float32


def staged_table():
    """the host's twiddle table (satools_amd/f0.py) and yaapt_stage_twiddles_kernel's layout of it: out[(h - 1) + p] = tw[p * (4096 / h)]"""
    k = np.arange(4096)
    tw = np.stack([np.cos(2 * np.pi * k / 8192.0), -np.sin(2 * np.pi * k / 8192.0)], 1).astype(f32)
    out = np.zeros((8191, 2), f32)
    h = 1
    while h <= 4096:
        out[h - 1:2 * h - 1] = tw[np.arange(h) * (4096 // h)]
        h *= 2
    return out


STW = staged_table()


def brev12(m):
    return sum(((m >> b) & 1) << (LOG - 1 - b) for b in range(LOG))


def copy_stages(L):
    lp = (L + 1) >> 1
    return 3 if lp <= N // 8 else 2 if lp <= N // 4 else 1 if lp <= N // 2 else 0


def load_map(L, threads=T):
    """-> (at [threads, rounds], m [threads, rounds], z): the element thread t writes in round k and the point it holds"""
    z = copy_stages(L)
    waves = threads // 64
    rounds = 64 // waves
    tid = np.arange(threads)
    lane, wave = tid & 63, tid >> 6
    r, q = lane & ((1 << z) - 1), (((lane & 31) >> z) << 1) | (lane >> 5)
    m = (q[:, None] << 6) | (wave[:, None] * rounds + np.arange(rounds)[None, :])
    return brev12(m) + r[:, None], m, z


def load_packed(fr, L):
    """fr [F, L] float32 -> (re, im [F, 4096], first stage left)"""
    at, m, z = load_map(L)
    x = np.zeros((fr.shape[0], 2 * N), f32)
    x[:, :L] = fr
    re, im = np.full((fr.shape[0], N), np.nan, f32), np.full((fr.shape[0], N), np.nan, f32)
    re[:, at.ravel()] = x[:, 2 * m.ravel()]
    im[:, at.ravel()] = x[:, 2 * m.ravel() + 1]
    return re, im, z + 1


def stages(re, im, first):
    F = re.shape[0]
    for s in range(first, LOG + 1):
        h = 1 << (s - 1)
        re, im = re.reshape(F, -1, 2, h), im.reshape(F, -1, 2, h)
        wx, wy = STW[h - 1:2 * h - 1, 0], STW[h - 1:2 * h - 1, 1]
        ar, ai, cr, ci = re[:, :, 0], im[:, :, 0], re[:, :, 1], im[:, :, 1]
        tr = cr * wx - ci * wy
        ti = cr * wy + ci * wx
        re, im = np.stack((ar + tr, ar - tr), 2), np.stack((ai + ti, ai - ti), 2)
        assert re.dtype == f32 and im.dtype == f32
    return re.reshape(F, N), im.reshape(F, N)


def untangle(re, im, k0, k1):
    """bins k0 .. k1 - 1 of the 8192-point transform, complex64 [F, k1 - k0]"""
    k = np.arange(max(k0, 1), k1)
    ar, ai, br, bi = re[:, k], im[:, k], re[:, N - k], im[:, N - k]
    er, ei = (ar + br) * f32(0.5), (ai - bi) * f32(0.5)
    pr, pi = (ai + bi) * f32(0.5), (br - ar) * f32(0.5)
    wx, wy = STW[N - 1 + k, 0], STW[N - 1 + k, 1]
    tr = pr * wx - pi * wy
    ti = pr * wy + pi * wx
    xr, xi = er + tr, ei + ti
    assert xr.dtype == f32 and xi.dtype == f32
    out = xr.astype(np.complex64) + 1j * xi.astype(np.complex64)
    if k0 == 0:
        out = np.concatenate(((re[:, :1] + im[:, :1]).astype(np.complex64), out), 1)
    return out


def packed_bins(fr, k0, k1):
    re, im, first = load_packed(fr, fr.shape[1])
    return untangle(*stages(re, im, first), k0, k1)


def ratio(fr, k0, k1):
    """largest |float32 bin - float64 bin| / running bound over bins k0 .. k1 - 1 of the frames fr [F, L] float32, taken as exact"""
    got = packed_bins(fr, k0, k1)
    X, E = r64.fft_running(fr.astype(np.float64), np.zeros(fr.shape), R, k1)
    err = np.abs(got.astype(np.complex128) - X[:, k0:k1])
    b = E[:, k0:k1] + r64.FLOOR
    return float((err / b).max())


def kernel_frames(wav, opts):
    """-> (plan, hann-windowed frames [nframes, frame_size], kaiser-windowed mean-free frames [nframes, nframe_size]), float32, as
    yaapt_nlfer_kernel and yaapt_spec_kernel form them (the mean: float32 of the float64 mean, within the kernel's few roundings of it;
    the samples are taken as given either way)"""
    n = wav.numel()
    plan = oy.Plan(n, opts)
    x = np.concatenate([np.zeros(plan.pad, f32), wav.numpy(), np.zeros(plan.pad, f32)])
    need = plan.nframe_size + (plan.nframes - 1) * plan.frame_jump
    filt = np.zeros((2, max(need, x.size)), f32)
    for sig, v in ((0, x), (1, x * x)):
        filt[sig, :x.size] = biquad.band_limit(v, int(plan.fs), plan.p["bp_low"], plan.p["bp_high"])
    hann, kaiser = r64.tables(plan)
    start = np.arange(plan.nframes) * plan.frame_jump
    a = filt[0][start[:, None] + np.arange(plan.frame_size)[None, :]] * hann
    xw = filt[1][start[:, None] + np.arange(plan.nframe_size)[None, :]] * kaiser
    b = xw - xw.astype(np.float64).mean(1, keepdims=True).astype(f32)
    assert a.dtype == f32 and b.dtype == f32
    return plan, a, b


def spec_bins(plan):
    return plan.min_shc * (plan.nharm + 1) + (plan.max_shc - plan.min_shc) * (plan.nharm + 1) + plan.wl - plan.half_wl


def thin(fr, keep=12):
    """the first, the last and evenly spaced frames in between (a catalogue tone repeats itself frame after frame), and the frames
    next to the largest change of level (a burst's onset and its end)"""
    F = fr.shape[0]
    if F <= keep:
        return fr
    level = np.abs(fr).sum(1)
    jump = int(np.argmax(np.abs(np.diff(level))))
    pick = set(np.linspace(0, F - 1, keep - 4).astype(int).tolist()) | {max(jump - 1, 0), jump, min(jump + 1, F - 1), min(jump + 2, F - 1)}
    return fr[sorted(pick)]


# ---- the load -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 559, 560, 1023, 1024, 1025, 1026, 1120, 1280, 2047, 2048, 2049, 4096, 4097, 8192])
@pytest.mark.parametrize("threads", [256, 512])
def test_load_writes_every_element_once_and_without_bank_conflicts(L, threads):
    at, m, z = load_map(L, threads)
    assert z == (3 if L <= 1024 else 2 if L <= 2048 else 1 if L <= 4096 else 0)
    assert np.array_equal(np.sort(at.ravel()), np.arange(N))                       # nothing left for a zero fill
    assert (m < (N >> z)).all() and ((L + 1) // 2 <= (N >> z))                     # every point of the frame is among them
    assert np.array_equal(at & ~((1 << z) - 1), brev12(m))                         # the point's block of 2^z copies
    half = at.reshape(threads // 32, 32, -1)                                       # [half wave, lane, round]
    for k in range(half.shape[2]):
        banks = np.sort(half[:, :, k] % 32, axis=1)
        assert (banks == np.arange(32)[None, :]).all()


def test_copy_stages_are_copies():
    """a point over its block of 2^z elements is what z radix-2 stages make of it next to zeros, bit for bit"""
    rng = np.random.default_rng(0)
    for L in (560, 1120, 1026, 2050):
        fr = rng.standard_normal((2, L)).astype(f32)
        re, im, first = load_packed(fr, L)
        assert not np.isnan(re).any() and not np.isnan(im).any() and first == copy_stages(L) + 1
        x = np.zeros((2, 2 * N), f32)
        x[:, :L] = fr
        m = np.arange(N)
        re0, im0 = np.zeros((2, N), f32), np.zeros((2, N), f32)
        re0[:, brev12(m)], im0[:, brev12(m)] = x[:, 2 * m], x[:, 2 * m + 1]
        for a, b in zip(stages(re, im, first), stages(re0, im0, 1)):
            assert np.array_equal(a, b)


def test_untangle_is_the_real_transform():
    """loose and independent of the bound: the packed route computes the 8192-point transform of the zero-padded frame, bin 0 and
    an odd length included"""
    rng = np.random.default_rng(1)
    for L in (559, 560, 1120, 1280):
        fr = rng.standard_normal((3, L)).astype(f32)
        got = packed_bins(fr, 0, 1300)
        want = np.fft.rfft(fr.astype(np.float64), 8192)[:, :1300]
        assert np.abs(got - want).max() < 1e-3 * np.abs(want).max()


# ---- the bound ------------------------------------------------------------------------------------------------------------
_SEEN = {}


@pytest.mark.parametrize("case", [c for c in yc.accepted() if not c.exact_only], ids=repr)
def test_catalogue_frames_stay_inside_the_running_bound(case):
    plan, a, b = kernel_frames(case.wav(), case.opts)
    ra = ratio(thin(a), plan.nl_lo, plan.nl_hi)
    rb = ratio(thin(b), 0, spec_bins(plan))
    _SEEN[case.name] = (ra, rb)
    print(f"\n{case.name}: error / bound  nlfer {ra:.3f}  spec {rb:.3f}")
    assert ra <= 1.0 and rb <= 1.0, (case, ra, rb)


# frame lengths on the edges of the load: the anonymizer's, packed lengths on and one past the copy-stage edges, an odd frame, the
# entry point's limit; and NLFER bins from 0 on (f0_min 0.1 Hz: nl_lo = -1 + round(0.2 / 16000 * 8192) = -1 is refused, 2 Hz gives 1)
EDGE_OPTS = [dict(frame_length=35.0), dict(frame_length=32.0), dict(frame_length=32.07), dict(frame_length=34.95), dict(frame_length=40.0),
             dict(frame_length=35.0, f0_min=2.0)]


@pytest.mark.parametrize("extra", EDGE_OPTS, ids=lambda e: "_".join(f"{k}{v}" for k, v in e.items()))
def test_edge_frame_lengths_stay_inside_the_running_bound(extra):
    opts = {**yc.OPTS, **extra}
    weak = yc.tone(8000).double() + 1e-4 * torch.sin(2 * np.pi * 240.0 * torch.arange(8000, dtype=torch.float64) / yc.SR)
    for wav in (yc.tone(8000), weak.float(), yc.noisy_tone(3, 8000)):
        plan, a, b = kernel_frames(wav, opts)
        assert plan.nl_lo >= 0
        ra, rb = ratio(thin(a, 8), plan.nl_lo, plan.nl_hi), ratio(thin(b, 8), 0, spec_bins(plan))
        print(f"\n{extra}: frame_size {plan.frame_size}  bins {plan.nl_lo}..{plan.nl_hi}  error / bound  nlfer {ra:.3f}  spec {rb:.3f}")
        assert ra <= 1.0 and rb <= 1.0, (extra, ra, rb)
