"""YAAPT on the HIP device under OTHER OPTION SETS than the anonymizer's one: the (case, set) pairs of tests/yaapt_cases.py
(OPTION_SETS), checked stage by stage with the functions of tests/test_hip_yaapt_stages.py and the plan of the set.  Needs a real
MI355X: run with `-m gpu` (`-s` prints the ratios).

Every other device test of YAAPT runs one plan: frame_size 560, frame_jump 320, tda_len 400 (overlap 80), nharm 3, median 7,
max_shc 256, wl 21, bins 60..205, sr 16000, every scalar at one value.  Here the plan moves: nframe_size 1280 with an overlap of
128, tda_len 1024, an overlap of 1, short frames, 8 kHz and 22.05 kHz, 1 / 4 / 6 harmonics, medians 1 / 3 / 5, other f0 and SHC
ranges, nccf_pwidth 9, other biquads, and one set per scalar option (the wiring sets: tests/test_yaapt_cases_host.py shows on the
CPU that each of them changes what the oracle returns on its signal, so a kernel that ignores the option fails here).

WHAT IS CHECKED per pair is what tests/test_hip_yaapt_stages.py checks: exact stages exact (filt with the set's sr, bp_low, bp_high;
vuv; spec_pitch and pitch_std; the six refined pitch and merit rows; the final track against the oracle chain and against the reference's own track of
tests/golden/fx_f0_options.npz, frame 0 exempt), bounded stages within the bounds tests/ref64_yaapt.py derives from the plan, with
the rounding counts DEVICE of that file: nothing new is fitted.  The counts were re-read for the plan fields: `fm_head` is 8 whatever
the overlap (two loads per lane cover the 128 the entry point admits), `fm_tail`, `sp_mean`, `nl_sum`, `shc_avg`, `pw` take their
term counts from the plan through ref64_yaapt, `shc_sum` is wl sequential adds; `dot` was stated as ceil(n / 4) + 2 but the first
accumulator also takes the n % 4 left-over terms: n // 4 + n % 4 + 2 (corrected there).

INDEXING UNDER THE PLANS' EXTREMES (read off csrc/yaapt.hip before the first run; the entry point's requirement that covers each):
  s_tail[2048]      frame_means: index k < tda_nframes <= nframes <= 2048 (`nframes` requirement)
  head(k, lane+64)  frame_means: two loads per lane reach 128 head samples = the largest overlap (`tda_len - frame_jump <= 128`)
  d / phi[1024]     nccf: j < tda_len <= 1024; a row reads d[lag_min + l + j] <= d[lag_max - 1 + N - 1] = d[tda_len - 2]; the peak scan
                    reads phi[i + 1] with i <= lag_max - c < tda_len (N > 0, else status 2) and phi[i - 1] with i >= lag_min + c >= 1
  mag[SPEC_MAGP]    spec / spec_peaks: i < n_mag = max_shc * (nharm + 1) + wl <= 1280 (its own requirement); the largest read of the SHC
                    loop is mag[max_shc * (nharm + 1) + wl - 1]
  s_shc[256]        spec_peaks: tid < 256 >= max_shc; the flank loops read s_shc[tid +- c] with lo + c + 1 <= tid <= hi - c, hi + 1 < 256
  kaiser / x        spec: j < nframe_size <= 5 * 256 (five rounds of 256 threads); x[f * jump + j] < need <= Lz
  FFT fill          fft8192_load_padded: j < 1024 (z = 3) or 2048 (z = 2) covers frame_size <= 640 and nframe_size <= 1280
  post_lds / dp_lds 53 and 63 bytes per frame: 2048 frames = 106 KB and 126 KB of the 160 KB the kernels are granted
  filt rows         Lz = max(L, need); nlfer reads (nframes - 1) * jump + frame_size <= L, nccf (tda_nframes - 1) * jump + tda_len <= L
                    (the entry point requires tda_nframes == nframes)

MEASURED on an MI355X: profiles/yaapt_option_error_ratios.txt."""
import ctypes as C
import os
import re
import time

import pytest
import torch

import test_hip_yaapt_stages as st
import yaapt_cases as yc

pytestmark = pytest.mark.gpu
DEV = st.DEV
_RATIOS, _EXEMPT, _T0 = {}, {}, time.time()


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    """the largest error / bound ratio per option set and stage, the exempted frames and the wall time, printed when the module is
    done (and written to the file SAT_YAAPT_OPTION_RATIOS names, if set)"""
    yield
    lines = [f"{k[0]:22s} {k[1]:8s} {r:8.4f}   at {case}" for k, (r, case) in sorted(_RATIOS.items())]
    lines.append("frames inside the float64 bound of a decision (exempt; `/unbounded`: no finite bound), per case and stage:"
                 + ("" if _EXEMPT else " none"))
    lines += [f"  {name}: {stages}" for name, stages in sorted(_EXEMPT.items())]
    lines.append(f"wall time of tests/test_hip_yaapt_options.py: {time.time() - _T0:.1f} s")
    print("\nYAAPT option sets: largest observed error / derived bound (a ratio above 1 fails)\n" + "\n".join(lines))
    path = os.environ.get("SAT_YAAPT_OPTION_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_yaapt_options.py: largest observed error / derived bound, per option set and stage (a ratio above 1 fails)\n")
            f.write("\n".join(lines) + "\n")


def _note(stage, case, res):
    st._note(stage, case, res, _RATIOS, _EXEMPT, key=(case.name.split("/")[0], stage))


@pytest.fixture(scope="module")
def fx(gold):
    return gold.npz("fx_f0_options.npz")


def _valid_call_is_unchanged(fx):
    """a following valid call gives its usual bits: no sticky state"""
    from satools_amd import f0 as f0_hip
    small = yc.option_set("ov1").cases[0]
    again = f0_hip.yaapt(small.wav().unsqueeze(0).to(DEV), small.opts).cpu()[0]
    torch.cuda.synchronize()
    assert torch.equal(again, st.device_run(small)[0])
    assert torch.equal(again[1:], torch.from_numpy(fx[small.name][0])[1:])


def _c_call(P, wav, dims=None):
    """sat_yaapt_f32 (or, with `dims` = the utt_dims rows, sat_yaapt_ragged_f32) called directly on sentinel-filled outputs
    -> (return code, last error, f0, status, workspace)"""
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    B = wav.shape[0]
    wav = wav.to(DEV).contiguous()
    hann, kaiser, tw = f0_hip._get_tables(P, wav.device)
    nws = _lib.lib().sat_yaapt_workspace_bytes(C.byref(P), B)
    ws = torch.zeros(nws // 4, device=DEV)
    f0 = torch.full((B, P.nframes), -7.0, device=DEV)
    status = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    tail = [_lib.ptr(f0), _lib.ptr(status), _lib.ptr(hann), _lib.ptr(kaiser), _lib.ptr(tw), _lib.ptr(ws), nws, B, _lib.stream()]
    if dims is None:
        rc = _lib.lib().sat_yaapt_f32(C.byref(P), _lib.ptr(wav), *tail)
    else:
        ud = torch.tensor(dims, dtype=torch.int32, device=DEV)
        rc = _lib.lib().sat_yaapt_ragged_f32(C.byref(P), _lib.ptr(wav), _lib.ptr(ud), *tail)
    torch.cuda.synchronize()
    return rc, _lib.lib().sat_last_error().decode(), f0.cpu(), status.cpu(), ws.cpu()


@pytest.mark.parametrize("case", yc.option_cases(), ids=repr)
def test_every_stage_under_the_option_set(case, fx):
    st.check_every_stage(case, fx, note=_note)


def test_status_2_where_the_reference_asserts(fx):
    """every NCCF window of the 120 Hz tone is empty under frame 10 / space 5 / tda 12 (N = tda_len - lag_max <= 0): the reference
    asserts (fixture), the plain call raises AssertionError with its message; deferred, in a batch of three, only the offending row
    is named and the other rows are their single tracks; nothing sticks"""
    from satools_amd import f0 as f0_hip
    s = yc.option_set("status2")
    bad, good = s.cases
    assert bad.raises == "AssertionError" and bool(fx["assert/" + bad.name]) and str(fx["raised/" + good.name]) == ""
    with pytest.raises(AssertionError, match="ERROR: Negative index in the cross correlation calculation of the pYAAPT time domain "
                                             "analysis. Please try to increase the value of the \"tda_frame_length\" parameter."):
        f0_hip.yaapt(bad.wav().unsqueeze(0).to(DEV), s.opts)
    one = st.device_run(good)[0]
    wav = torch.stack([good.wav(), bad.wav(), good.wav()]).to(DEV)
    f0, status = f0_hip.yaapt(wav, s.opts, defer_status=True)
    with pytest.raises(AssertionError, match=r"utterance\(s\) \[1\]\]"):
        status.check()
    assert status.words.tolist() == [0, 2, 0]
    for i in (0, 2):
        assert torch.equal(f0[i].cpu(), one), i
    wav = torch.stack([bad.wav(), good.wav(), bad.wav()]).to(DEV)
    f0, status = f0_hip.yaapt(wav, s.opts, defer_status=True)
    with pytest.raises(AssertionError, match=r"utterance\(s\) \[0, 2\]\]"):
        status.check()
    assert torch.equal(f0[1].cpu(), one)
    _valid_call_is_unchanged(fx)


def test_status_3_where_the_lag_window_is_empty(fx):
    """seven harmonics and f0_max 200: the SHC of the 120 Hz tone peaks at its octave, the spectral pitch lies above f0_max by more
    than two deviations and lag_max < lag_min.  The reference fails in crs_corr (RuntimeError, fixture); the device used to run a
    loop of negative length and return a track.  Now the NCCF kernel reports status 3 and the call raises RuntimeError"""
    from satools_amd import f0 as f0_hip
    s = yc.option_set("nharm7_f0max200")
    bad = s.cases[0]
    assert str(fx["raised/" + bad.name]) == "RuntimeError" and not bool(fx["assert/" + bad.name])
    with pytest.raises(RuntimeError, match=r"yaapt: the reference fails in a tensor operation on utterance\(s\) \[0\]: an empty lag window"):
        f0_hip.yaapt(bad.wav().unsqueeze(0).to(DEV), s.opts)
    _valid_call_is_unchanged(fx)


@pytest.mark.parametrize("s", yc.refused_sets(), ids=repr)
def test_refused_option_sets(s, fx):
    """each set outside the entry point's region raises SatError with the message of its requirement; the C entry points, handed the
    plan directly, return an error with that message and launch nothing (f0, status and a zeroed workspace keep their fill: the
    first thing a launch sequence does is to clear the status words); the next valid call is unchanged"""
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    case = s.cases[0]
    P = f0_hip._derive_plan(case.n, dict(s.opts))
    for dims in (None, [f0_hip.length_dims(P, case.n)]):
        rc, msg, f0, status, ws = _c_call(P, case.wav().unsqueeze(0), dims)
        assert rc != 0 and re.search(s.refused, msg), (rc, msg)
        assert bool((f0 == -7.0).all()) and int(status[0]) == -7 and not ws.any()
    with pytest.raises(_lib.SatError, match=s.refused):
        f0_hip.yaapt(case.wav().unsqueeze(0).to(DEV), s.opts)
    with pytest.raises(_lib.SatError, match=s.refused):
        f0_hip.yaapt_ragged(case.wav().unsqueeze(0).to(DEV), [case.n], s.opts)
    _valid_call_is_unchanged(fx)


def test_ragged_rows_the_reference_fails_on_or_the_kernels_cannot_do(fx):
    """under frame 40 / space 56 / tda 64 about two lengths in five have a negative zero extension (the reference fails: fixture of
    `space_gt_frame`) or fewer tda frames than analysis frames (the entry point refuses a single utterance of such a length: the NCCF
    kernel would read frame means that were never written).  f0.yaapt_ragged refuses such rows by name before the launch.  The C
    entry point sees only the plan of the longest row: its kernels flag the rows, status 3 and 4, and the good row is its single
    track; F0Status.check raises for each"""
    from oracle import yaapt as oy
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    s = yc.option_set("tda1024")
    good = s.cases[0]
    n_short, n_odd = 20480, 20 * 896 + 100          # need < L;  20 tda frames for 21 analysis frames
    p_short, p_odd = oy.Plan(n_short, s.opts), oy.Plan(n_odd, s.opts)
    assert p_short.need < p_short.L and p_odd.need >= p_odd.L and p_odd.tda_nframes == p_odd.nframes - 1
    assert str(fx["raised/space_gt_frame/tone_20480"]) == "RuntimeError"
    batch = torch.zeros(3, good.n)
    batch[0], batch[1, :n_short], batch[2, :n_odd] = good.wav(), yc.tone(n_short), yc.tone(n_odd)
    lens = [good.n, n_short, n_odd]
    with pytest.raises(_lib.SatError, match=r"yaapt_ragged: utterance\(s\) \[1\]: frame_space too long for frame_length"):
        f0_hip.yaapt_ragged(batch.to(DEV), lens, s.opts)
    with pytest.raises(_lib.SatError, match=r"yaapt_ragged: utterance\(s\) \[1\]: tda frame count differs from the analysis frame count"):
        f0_hip.yaapt_ragged(batch[[0, 2]].to(DEV), [good.n, n_odd], s.opts)
    P = f0_hip.make_plan(good.n, dict(s.opts))
    rc, msg, f0, status, _ = _c_call(P, batch, [f0_hip.length_dims(P, n) for n in lens])
    assert rc == 0, msg
    assert status.tolist() == [0, 3, 4]
    assert torch.equal(f0[0], st.device_run(good)[0])
    for code, exc, text in ((3, RuntimeError, "negative zero extension"), (4, _lib.SatError, r"tda frame count differs .* utterance\(s\) \[0\]")):
        word = torch.tensor([code], dtype=torch.int32, device=DEV)
        with pytest.raises(exc, match=text):
            f0_hip.F0Status(word, 1).check()
    _valid_call_is_unchanged(fx)


# ---- ragged batches ------------------------------------------------------------------------------------------------------
def _ragged_rows(name):
    """4, 63, 64, 65 and 129 frames of the set's jump, the clipped case, a burst"""
    s = yc.option_set(name)
    jump = int(s.opts["frame_space"] * s.opts.get("sr", yc.SR) / 1000)
    return [s._case(sig) for sig in (("tone", 4 * jump), ("tone", 63 * jump), ("tone", 64 * jump), ("tone", 64 * jump + 1), ("tone", 129 * jump),
                                     ("clip40", 63 * jump), ("burst", 3 * jump, 40 * jump, 50 * jump))]


@pytest.mark.parametrize("B", [7, 33])
@pytest.mark.parametrize("name", ["jump512_ov128", "sr22050"])
def test_ragged_batch_rows_are_their_single_tracks(name, B):
    """zero past each row's frames, bit for bit the single-utterance track.  33 rows: a second prefilter block of 32 and (one pad
    sample under the 16 kHz set; 22.05 kHz has an odd padding anyway) the unaligned row path"""
    from oracle import yaapt as oy
    from satools_amd import f0 as f0_hip
    rows = _ragged_rows(name)
    cases = [rows[i % len(rows)] for i in range(B)]
    n_max = max(c.n for c in cases) + (1 if B == 33 else 0)
    wav = torch.zeros(B, n_max)
    for i, c in enumerate(cases):
        wav[i, :c.n] = c.wav()
    opts = cases[0].opts
    got = f0_hip.yaapt_ragged(wav.to(DEV), [c.n for c in cases], opts).cpu()
    assert got.shape == (B, oy.Plan(n_max, opts).nframes)
    assert [c.nframes for c in rows[:5]] == [4, 63, 64, 65, 129]
    assert not torch.isnan(got).any()
    for i, c in enumerate(cases):
        one, _ = st.device_run(c)
        assert torch.equal(got[i, :c.nframes], one), (i, c, torch.nonzero(got[i, :c.nframes] != one).flatten()[:8].tolist())
        assert not got[i, c.nframes:].any(), (i, c)
