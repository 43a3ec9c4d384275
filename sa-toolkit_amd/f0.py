"""YAAPT F0 extraction on the HIP device behind the reference's `yaapt(wav, opts)` call
(satools/satools/hifigan/yaapt.py:946-951; options as passed by
egs/vc/libritts/local/tuning/hifigan.py:31-36).

The host derives the integer/scalar plan exactly the way the reference derives it from its
option dict (Python float arithmetic, math.floor/ceil, torch f32 rounds where the reference uses
them) and builds the three tables (hann, kaiser, FFT twiddles); everything else runs in
sat_yaapt_f32.  Unlike the reference (serial over the batch, forced to the CPU, yaapt.py:798-799)
the whole batch is processed in one call on the GPU."""
import ctypes as C
import functools
import math
import threading

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream

DEFAULTS = dict(sr=16000.0, frame_length=35.0, tda_frame_length=35.0, frame_space=10.0, f0_min=60.0, f0_max=400.0,
                fft_length=8192.0, bp_low=50.0, bp_high=1500.0, nlfer_thresh1=0.75, nlfer_thresh2=0.1,
                shc_numharms=3.0, shc_window=40.0, shc_maxpeaks=4.0, shc_pwidth=50.0, shc_thresh1=5.0,
                shc_thresh2=1.25, f0_double=150.0, f0_half=150.0, dp5_k1=11.0, nccf_thresh1=0.3,
                nccf_thresh2=0.9, nccf_maxcands=3.0, nccf_pwidth=5.0, merit_boost=0.20, merit_pivot=0.99,
                merit_extra=0.4, median_value=7.0, dp_w1=0.15, dp_w2=0.5, dp_w3=0.1, dp_w4=0.9,
                spec_pitch_min_std=0.05)  # yaapt.py:815-859


# frame_space > frame_length can leave the last spectral frame (2 * frame_size samples from the last frame's start) inside the padded
# signal: the reference then asks torch.zeros for a negative zero extension (yaapt.py:206-210) and fails with a RuntimeError
NEGATIVE_EXTENSION = ("yaapt: frame_space too long for frame_length: the last spectral frame ends at sample %d of the %d padded ones "
                      "(the reference fails on the negative zero extension of spec_track)")


class YaaptPlan(C.Structure):
    """mirror of sat_yaapt_plan (include/satools_hip.h)"""
    _fields_ = [(k, C.c_int32) for k in (
        "n", "pad", "L", "Lz", "nfft", "frame_size", "frame_jump", "nframes", "nl_lo", "nl_hi", "nframe_size",
        "half_wl", "wl", "max_shc", "min_shc", "nharm", "maxpeaks", "pk_center", "pk_min_lag", "pk_max_lag",
        "tda_len", "tda_nframes", "maxcands", "nccf_center", "median_value")] + [(k, C.c_float) for k in (
        "fs", "delta", "nlfer_thresh1", "nlfer_thresh2", "shc_thresh1", "inv_shc_thresh1", "shc_thresh2",
        "f0_double", "f0_half", "merit_extra", "dp5_k1", "f0_min", "f0_max", "spec_pitch_min_std",
        "nccf_thresh1", "nccf_thresh2", "merit_boost1", "merit_pivot", "dp_w1", "dp_w2", "dp_w3", "dp_w4")] + [
        ("lp", C.c_float * 6), ("hp", C.c_float * 6)]


@functools.lru_cache(maxsize=64)
def biquad_constants(kind, sample_rate, cutoff, Q=0.707):
    """RBJ biquad as torchaudio.functional.{lowpass,highpass}_biquad computes it (f32 tensors), then
    the normalisation `_lfilter` applies FIRST to both coefficient vectors: {b0/a0, b1/a0, b2/a0, a0, a1/a0, a2/a0}
    (f32 divisions; a0 itself is unused by the kernel).  torchaudio is third-party to the reference
    (yaapt.py:46-47) and absent here: restated from its published algorithm, the FIR order a tested decision
    (oracle/biquad.py, tests/golden/fx_biquad_order.json)."""
    f32 = torch.float32
    w0 = 2 * math.pi * torch.as_tensor(cutoff, dtype=f32) / sample_rate
    alpha = torch.sin(w0) / 2 / torch.as_tensor(Q, dtype=f32)
    if kind == "lp":
        b0 = (1 - torch.cos(w0)) / 2
        b1 = 1 - torch.cos(w0)
    else:
        b0 = (1 + torch.cos(w0)) / 2
        b1 = -1 - torch.cos(w0)
    a0, a1, a2 = 1 + alpha, -2 * torch.cos(w0), 1 - alpha
    v = np.array([float(b0), float(b1), float(b0), float(a0), float(a1), float(a2)], dtype=np.float32)
    return [float(np.float32(v[0] / v[3])), float(np.float32(v[1] / v[3])), float(np.float32(v[2] / v[3])), float(v[3]),
            float(np.float32(v[4] / v[3])), float(np.float32(v[5] / v[3]))]


def make_plan(n, opts):
    """the plan of `opts` at n samples.  Raises where the reference fails for every signal of that length (a negative zero
    extension); every other limit is the entry point's to refuse"""
    P = _derive_plan(n, opts)
    need = P.nframe_size + (P.nframes - 1) * P.frame_jump
    if need < P.L:
        raise _lib.SatError(NEGATIVE_EXTENSION % (need, P.L))
    return P


def _derive_plan(n, opts):
    p = dict(DEFAULTS)
    if "frame_lengtht" in opts and "tda_frame_length" not in opts:   # yaapt.py:802-810
        opts = dict(opts)
        opts["tda_frame_length"] = opts.pop("frame_lengtht")
    p.update(opts)
    fs = p["sr"]
    P = YaaptPlan()
    P.n = n
    P.pad = int(p["frame_length"] / 1000 * int(p["sr"])) // 2                       # yaapt.py:868
    P.L = n + 2 * P.pad
    P.nfft = int(p["fft_length"])
    P.frame_size = int(math.floor(p["frame_length"] * fs / 1000))                  # :882
    P.frame_jump = int(math.floor(p["frame_space"] * fs / 1000))                   # :883
    half = P.frame_size // 2
    P.nframes = len(range(half, P.L - half, P.frame_jump))                         # nlfer :163-165
    P.nl_lo = int(torch.round(torch.tensor(p["f0_min"] * 2 / float(fs)) * P.nfft)) - 1   # :156, slice start N-1
    P.nl_hi = int(torch.round(torch.tensor(p["f0_max"] / float(fs)) * P.nfft))          # :157
    P.nframe_size = P.frame_size * 2                                               # spec_track :189
    delta = fs / P.nfft
    wl = math.floor(p["shc_window"] / delta)
    P.half_wl = math.floor(float(wl) / 2)
    P.wl = wl + 1 if wl % 2 == 0 else wl
    P.max_shc = math.floor((p["f0_max"] + p["shc_pwidth"] * 2) / delta)
    P.min_shc = math.ceil(p["f0_min"] / delta)
    P.nharm = int(p["shc_numharms"])
    P.maxpeaks = int(p["shc_maxpeaks"])
    w = math.floor(p["shc_pwidth"] / delta)                                        # peaks :396-406
    width = w + 1 if w % 2 == 0 else w
    P.pk_center = math.ceil(width / 2)
    P.pk_min_lag = max(1, math.floor(p["f0_min"] / delta - P.pk_center))
    P.pk_max_lag = min(math.floor(p["f0_max"] / delta + P.pk_center), P.max_shc - width)
    P.tda_len = int(p["tda_frame_length"] * fs / 1000)                             # time_track :686-694
    P.tda_nframes = min(int((P.L - (P.tda_len - P.frame_jump)) / P.frame_jump), P.nframes)
    P.maxcands = int(p["nccf_maxcands"])
    P.nccf_center = math.floor(p["nccf_pwidth"] / 2.0)
    P.median_value = int(p["median_value"])
    need = P.nframe_size + (P.nframes - 1) * P.frame_jump                          # zero extension, :206-210
    P.Lz = max(P.L, need)
    P.fs, P.delta = fs, delta
    for k in ("nlfer_thresh1", "nlfer_thresh2", "shc_thresh1", "shc_thresh2", "f0_double", "f0_half", "merit_extra",
              "dp5_k1", "f0_min", "f0_max", "spec_pitch_min_std", "nccf_thresh1", "nccf_thresh2", "merit_pivot",
              "dp_w1", "dp_w2", "dp_w3", "dp_w4"):
        setattr(P, k, p[k])
    P.inv_shc_thresh1 = 1 / p["shc_thresh1"]
    P.merit_boost1 = 1 + p["merit_boost"]
    lp = biquad_constants("lp", int(fs), p["bp_low"])
    hp = biquad_constants("hp", int(fs), p["bp_high"])
    for i in range(6):
        P.lp[i], P.hp[i] = lp[i], hp[i]
    return P


def length_dims(P, n):
    """[n, L, nframes, tda_nframes] of make_plan(n, opts) from a plan P of the same options at another length: the only fields of a
    plan that depend on the length (a ragged batch of 32 lengths was 32 full plans, 4 ms of host time per batch in the batch job's
    launching thread; tests/test_host_logic.py holds the two against each other)"""
    L = n + 2 * P.pad
    half = P.frame_size // 2
    nframes = len(range(half, L - half, P.frame_jump))
    return [n, L, nframes, min(int((L - (P.tda_len - P.frame_jump)) / P.frame_jump), nframes)]


_tables = {}


def _get_tables(P, device):
    key = (P.frame_size, str(device))
    if key not in _tables:
        hann = torch.hann_window(P.frame_size + 2)[1:-1].contiguous()              # nlfer :159
        kaiser = torch.kaiser_window(P.nframe_size, periodic=True, beta=0.5)       # spec_track :213
        k = np.arange(4096, dtype=np.float64)
        tw = np.stack([np.cos(2 * np.pi * k / 8192.0), -np.sin(2 * np.pi * k / 8192.0)], 1).astype(np.float32)
        _tables[key] = (hann.to(device), kaiser.to(device), torch.from_numpy(tw).to(device))
    return _tables[key]


class _PinnedInts:
    """rows of ONE page-locked int32 block for the words that travel with a yaapt launch (its status, the per-utterance dimensions of a
    ragged batch).  A `tensor.pin_memory()` per call asks torch's host allocator for a block whose previous copy has completed; a
    launching thread that runs ahead of the GPU (the batch job with deferred status) finds none and pays a hipHostMalloc per launch,
    ~50 ms each at the start of a job (0.67 s for the first four batches)."""
    ROWS, COLS = 64, 1024

    def __init__(self):
        self.buf, self.free, self.lock = None, list(range(self.ROWS)), threading.Lock()

    def take(self, n):
        """-> (pinned int32 view of n words, row to give back or None)"""
        with self.lock:
            if self.buf is None:
                self.buf = torch.empty(self.ROWS, self.COLS, dtype=torch.int32, pin_memory=True)
            row = self.free.pop() if (self.free and n <= self.COLS) else None
        if row is None:
            return torch.empty(n, dtype=torch.int32).pin_memory(), None
        return self.buf[row, :n], row

    def give(self, row):
        if row is not None:
            with self.lock:
                self.free.append(row)


_pinned_ints = _PinnedInts()


class F0Status:
    """deferred error report of one yaapt launch (checked without stalling the launch stream); `also` = rows of _pinned_ints that the
    launch read (a ragged batch's dimensions), free once the status has arrived"""

    def __init__(self, dev_status, B, also=()):
        self.host, row = _pinned_ints.take(B)
        self.rows = [row] + list(also)
        self.host.copy_(dev_status, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def _release(self):
        rows, self.rows = self.rows, []
        for r in rows:
            _pinned_ints.give(r)

    def __del__(self):
        try:
            if self.rows:
                self.event.synchronize()        # (never checked: the copies must have landed before the rows are reused)
                self._release()
        except Exception:
            pass

    def check(self):
        if self.host is not None:
            self.event.synchronize()
            self.words, self.host = self.host.clone(), None
            self._release()
        st = self.words
        if (st == 1).any():
            # the reference fails inside medfilt/unfold when no frame of an utterance is voiced
            raise RuntimeError("yaapt: no voiced frame in utterance(s) %s (the reference's spec_track fails on an "
                               "empty candidate list)" % (st == 1).nonzero().flatten().tolist())
        if (st == 4).any():
            # only through the C ABI's ragged form: yaapt_ragged refuses such rows before the launch
            raise _lib.SatError("yaapt: tda frame count differs from the analysis frame count in utterance(s) %s"
                                % (st == 4).nonzero().flatten().tolist())
        if (st == 3).any():
            # the reference fails in a tensor operation: as_strided with lag_max - lag_min < 0 rows in crs_corr's stride_matrix
            # (yaapt.py:594) when the spectral pitch lies outside [f0_min, f0_max] by more than two deviations; or (through the C ABI's
            # ragged form only) torch.zeros of a negative zero extension (:206-210)
            raise RuntimeError("yaapt: the reference fails in a tensor operation on utterance(s) %s: an empty lag window (lag_max < lag_min, "
                               "the spectral pitch lies outside f0_min..f0_max by more than two deviations) or a negative zero extension"
                               % (st == 3).nonzero().flatten().tolist())
        if (st == 2).any():
            raise AssertionError("ERROR: Negative index in the cross correlation calculation of the pYAAPT time domain "
                                 "analysis. Please try to increase the value of the \"tda_frame_length\" parameter."
                                 " [yaapt: utterance(s) %s]" % (st == 2).nonzero().flatten().tolist())


def workspace_views(ws, P, B):
    """named views into the sat_yaapt_f32 workspace (layout of csrc/yaapt.hip), for diagnostics/tests"""
    nf, Lz = P.nframes, P.Lz
    out, off = {}, 0
    for name, shape, dt in (("filt", (B, 2, Lz), torch.float32), ("e_raw", (B, nf), torch.float32),
                            ("energy", (B, nf), torch.float32), ("vuv", (B, nf), torch.int32),
                            ("cand", (B, 8, nf), torch.float32), ("spec_pitch", (B, nf), torch.float32),
                            ("scal", (B, 4), torch.float32), ("fmean", (B, 2, nf), torch.float32),
                            ("tp", (B, 2, nf), torch.float32), ("tm", (B, 2, nf), torch.float32),
                            ("refined", (B, 12, nf), torch.float32)):       # refine(): pitch[6], merit[6]
        cnt = int(np.prod(shape))
        out[name] = ws[off:off + cnt].view(dt).view(*shape)
        off += cnt
    return out


def yaapt_ragged(wav, lengths, opts, defer_status=False):
    """wav [B, n_max] zero-padded on the HIP device, lengths [B] -> F0 [B, nframes(n_max)]: every utterance tracked
    at its own length (zero past its frames), all in one launch sequence"""
    if not wav.is_cuda or wav.dim() != 2:
        raise _lib.SatError("yaapt_ragged expects [B, samples] on the HIP device")
    wav = wav.to(torch.float32).contiguous()
    B, n_max = wav.shape
    lens = [int(v) for v in lengths]
    if len(lens) != B or max(lens) > n_max or min(lens) <= 0:
        raise _lib.SatError("yaapt_ragged: lengths do not fit the batch")
    P = make_plan(n_max, dict(opts))
    dims = [length_dims(P, n) for n in lens]
    if max(d[2] for d in dims) > P.nframes or max(d[1] for d in dims) > P.Lz:
        raise _lib.SatError("yaapt_ragged: an utterance exceeds the batch plan")
    short = [i for i, d in enumerate(dims) if P.nframe_size + (d[2] - 1) * P.frame_jump < d[1]]
    if short:      # like make_plan, per utterance: the reference fails on each of them
        d = dims[short[0]]
        raise _lib.SatError("yaapt_ragged: utterance(s) %s: " % short + NEGATIVE_EXTENSION[7:] % (P.nframe_size + (d[2] - 1) * P.frame_jump, d[1]))
    odd = [i for i, d in enumerate(dims) if d[3] != d[2]]
    if odd:        # as the entry point requires of a single utterance (tda_frame_length above frame_length, at some lengths)
        raise _lib.SatError("yaapt_ragged: utterance(s) %s: tda frame count differs from the analysis frame count" % odd)
    hann, kaiser, tw = _get_tables(P, wav.device)
    ws_bytes = lib().sat_yaapt_workspace_bytes(C.byref(P), B)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=wav.device)
    f0 = torch.empty(B, P.nframes, dtype=torch.float32, device=wav.device)
    status = torch.empty(B, dtype=torch.int32, device=wav.device)
    ud_host, ud_row = _pinned_ints.take(4 * B)
    ud_host.copy_(torch.tensor(dims, dtype=torch.int32).reshape(-1))
    ud = ud_host.to(wav.device, non_blocking=True).view(B, 4)
    check(lib().sat_yaapt_ragged_f32(C.byref(P), ptr(wav), ptr(ud), ptr(f0), ptr(status), ptr(hann), ptr(kaiser), ptr(tw),
                                     ptr(ws), ws_bytes, B, stream()), "sat_yaapt_ragged_f32")
    st = F0Status(status, B, also=(ud_row,))
    if defer_status:
        return f0, st
    st.check()
    return f0


MAX_RESIDENT_FRAMES = 2048      # sat_yaapt_f32 / sat_yaapt_ragged_f32: a block's LDS holds the whole utterance (csrc/yaapt_dev.h)
LONG_CHUNK_STEP, LONG_DEFAULT_CHUNK, LONG_MAX_CHUNK = 64, 1024, 2048     # include/satools_hip_yaapt_long.h


def plan_frames(n, opts):
    """make_plan(n, opts).nframes from the three options it depends on, in plain Python (the dispatch of `track` runs on every call of
    the batch job's launching thread; a whole plan costs torch calls).  tests/test_yaapt_long_host.py holds the two against each other."""
    g = lambda k: opts.get(k, DEFAULTS[k])
    sr = g("sr")
    pad = int(g("frame_length") / 1000 * int(sr)) // 2
    half = int(math.floor(g("frame_length") * sr / 1000)) // 2
    return len(range(half, n + 2 * pad - half, int(math.floor(g("frame_space") * sr / 1000))))


MAX_RESIDENT_OVERLAP = 128      # sat_yaapt_f32 / sat_yaapt_ragged_f32: tda_len - frame_jump (yaapt_check_plan, csrc/yaapt.hip)
LONG_MAX_DEPTH = 7              # sat_yaapt_long_f32: the earlier frames a frame may overlap, ceil(tda_len / frame_jump) - 1


def plan_overlap(opts):
    """tda_len - frame_jump of make_plan(n, opts) (no length enters) in plain Python, for the dispatch of `track` like `plan_frames`:
    above MAX_RESIDENT_OVERLAP a frame of time_track overlaps more than the resident kernels subtract means for (the reference's own
    defaults: 560 - 160 = 400) and the batch goes to the long form, which has kernels for it"""
    g = lambda k: opts.get(k, DEFAULTS[k])
    tda = opts["frame_lengtht"] if ("frame_lengtht" in opts and "tda_frame_length" not in opts) else g("tda_frame_length")
    sr = g("sr")
    return int(tda * sr / 1000) - int(math.floor(g("frame_space") * sr / 1000))


def long_frames_ok(P):
    """whether sat_yaapt_long_f32 takes the plan's length: the prefilter kernel's 31-bit row offsets (about 26 200 frames at a 20 ms hop)"""
    return 32 * P.n * 4 < 2 ** 31 and 64 * P.Lz * 4 < 2 ** 31 and P.nframes <= 32767


def yaapt_long(wav, opts, lengths=None, chunk_frames=0, defer_status=False, return_aux=False):
    """`yaapt` (lengths None) and `yaapt_ragged` in one function, for any frame count from 4 up to the prefilter's limit
    (sat_yaapt_long_f32): the per-utterance stages walk the frames in chunks of `chunk_frames` (0 = the default, else a multiple of 64 up to
    2048) instead of holding the utterance in one block's LDS.  Same arithmetic in the same order: up to 2048 frames the result has the bits
    of `yaapt` / `yaapt_ragged`.  Also the only form for options whose frames overlap by more than 128 samples (up to LONG_MAX_DEPTH earlier
    frames: the reference's defaults overlap three).  return_aux: also the named views of the workspace's head (`workspace_views`)."""
    if not wav.is_cuda:
        raise _lib.SatError("yaapt_long runs on the HIP device only (no CPU fallback); move the input to 'cuda'")
    if wav.dim() != 2:
        raise _lib.SatError("yaapt_long expects [B, samples]")
    wav = wav.to(torch.float32).contiguous()
    B, n_max = wav.shape
    P = make_plan(n_max, dict(opts))
    ud, also = None, ()
    if lengths is not None:
        lens = [int(v) for v in lengths]
        if len(lens) != B or max(lens) > n_max or min(lens) <= 0:
            raise _lib.SatError("yaapt_long: lengths do not fit the batch")
        dims = [length_dims(P, n) for n in lens]
        if max(d[2] for d in dims) > P.nframes or max(d[1] for d in dims) > P.Lz:
            raise _lib.SatError("yaapt_long: an utterance exceeds the batch plan")
        short = [i for i, d in enumerate(dims) if P.nframe_size + (d[2] - 1) * P.frame_jump < d[1]]
        if short:      # like make_plan, per utterance: the reference fails on each of them
            d = dims[short[0]]
            raise _lib.SatError("yaapt_long: utterance(s) %s: " % short + NEGATIVE_EXTENSION[7:] % (P.nframe_size + (d[2] - 1) * P.frame_jump, d[1]))
        odd = [i for i, d in enumerate(dims) if d[3] != d[2]]
        if odd:        # as the entry point requires of a single utterance (tda_frame_length above frame_length, at some lengths)
            raise _lib.SatError("yaapt_long: utterance(s) %s: tda frame count differs from the analysis frame count" % odd)
    hann, kaiser, tw = _get_tables(P, wav.device)
    ws_bytes = lib().sat_yaapt_long_workspace_bytes(C.byref(P), B, int(chunk_frames))
    if not long_frames_ok(P):
        ws_bytes = 256          # the entry point refuses the plan by name before it looks at the workspace: nothing that large is allocated
    ws = torch.empty(max(ws_bytes, 256) // 4, dtype=torch.float32, device=wav.device)
    f0 = torch.empty(B, P.nframes, dtype=torch.float32, device=wav.device)
    status = torch.empty(B, dtype=torch.int32, device=wav.device)
    if lengths is not None:
        ud_host, ud_row = _pinned_ints.take(4 * B)
        ud_host.copy_(torch.tensor(dims, dtype=torch.int32).reshape(-1))
        ud = ud_host.to(wav.device, non_blocking=True).view(B, 4)
        also = (ud_row,)
    try:
        check(lib().sat_yaapt_long_f32(C.byref(P), ptr(wav), ptr(ud), ptr(f0), ptr(status), ptr(hann), ptr(kaiser), ptr(tw), ptr(ws),
                                       ws_bytes, B, int(chunk_frames), stream()), "sat_yaapt_long_f32")
    except _lib.SatError:
        if also:                 # refused before any launch: wait for the table's copy, then its pinned row is free again
            torch.cuda.current_stream().synchronize()
            _pinned_ints.give(also[0])
        raise
    st = F0Status(status, B, also=also)
    if defer_status:
        return f0, st
    st.check()
    if return_aux:
        return f0, workspace_views(ws, P, B)
    return f0


def track(wav, opts, lengths=None, defer_status=False):
    """the F0 of a batch at any length the device takes: a batch plan of up to MAX_RESIDENT_FRAMES frames goes to `yaapt` (lengths None) or
    `yaapt_ragged` exactly as before, a longer one to `yaapt_long` (every row of a ragged batch then: the rows' results are the same
    bits either way).  Options whose frames overlap by more than MAX_RESIDENT_OVERLAP samples (the reference's defaults, a 10 ms hop) go to
    `yaapt_long` at every length: its wide kernels alone serve them.
    What Net.get_f0 / get_f0_ragged / convert / convert_padded and the batch job call."""
    if plan_overlap(opts) <= MAX_RESIDENT_OVERLAP and plan_frames(wav.shape[-1], opts) <= MAX_RESIDENT_FRAMES:
        if lengths is None:
            return yaapt(wav, opts, defer_status=defer_status)
        return yaapt_ragged(wav, lengths, opts, defer_status=defer_status)
    return yaapt_long(wav, opts, lengths=lengths, defer_status=defer_status)


def yaapt(wav, opts, defer_status=False, return_aux=False):
    """wav [B, n] on the HIP device -> F0 [B, nframes] on the same device"""
    if not wav.is_cuda:
        raise _lib.SatError("yaapt runs on the HIP device only (no CPU fallback); move the input to 'cuda'")
    if wav.dim() != 2:
        raise _lib.SatError("yaapt expects [B, samples]")
    wav = wav.to(torch.float32).contiguous()
    B, n = wav.shape
    P = make_plan(n, dict(opts))
    hann, kaiser, tw = _get_tables(P, wav.device)
    ws_bytes = lib().sat_yaapt_workspace_bytes(C.byref(P), B)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=wav.device)
    f0 = torch.empty(B, P.nframes, dtype=torch.float32, device=wav.device)
    status = torch.empty(B, dtype=torch.int32, device=wav.device)
    check(lib().sat_yaapt_f32(C.byref(P), ptr(wav), ptr(f0), ptr(status), ptr(hann), ptr(kaiser), ptr(tw), ptr(ws),
                              ws_bytes, B, stream()), "sat_yaapt_f32")
    st = F0Status(status, B)
    if defer_status:
        return f0, st
    st.check()
    if return_aux:
        return f0, workspace_views(ws, P, B)
    return f0
