"""Input catalogue of the long-form YAAPT tests (sat_yaapt_long_f32, tests/test_hip_yaapt_long.py): utterances BEYOND the 2048 frames of
sat_yaapt_f32, built from the generators of tests/yaapt_cases.py, each with the properties it is there for (asserted from the float32
oracle by tests/test_yaapt_long_host.py, and held against the reference's own tracks in tests/golden/fx_f0_long.npz, written by
tests/golden/make_f0_long_fixtures.py).

  tone_655361          2049 frames: one frame past the resident kernels, the smallest long case
  noisy1_655361        the same length under noise: NCCF decisions and median outliers on every chunk
  gated2_660000        noisy_tone(2) gated 3 s on / 1 s off, 2063 frames: well under half the frames carry a spectral candidate, so the
                       compacted axis of spec_track (its Viterbi, medians and float64 sums) and the frame axis have different chunk edges,
                       and runs of unvoiced frames cross them
  jump_700000          150 Hz then 100 Hz, 2188 frames: the Viterbi costs decide around the switch
  gated2_1310721       the gated signal at 4097 frames: a fifth chunk of one frame at the default chunk of 1024
  noisy1_2621441       8193 frames (checked against the fixture only: the float32 oracle of the later stages is slow at that length)
  burst60_..           a 60-sample burst in 655361 samples: frames above the NLFER threshold, none with a spectral candidate (nv = 0):
                       the reference raises, the device reports status 1
  burst270_..          nv = 2 in 2049 frames: the constant-150-Hz branch (no Viterbi in spec_track), a NaN mean_pitch in dynamic()

Also here: `walk`, the chunk walk of csrc/yaapt_long/yaapt_long.hip restated in plain Python (which frames a chunk stages, with which
halo, and what it carries to the next one), for the host test that pins its constants to the source."""
import math

import torch

import yaapt_cases as yc

OPTS = yc.OPTS
MAX_RESIDENT = yc.MAX_FRAMES          # 2048
CHUNK_STEP, DEFAULT_CHUNK, MAX_CHUNK, HALO = 64, 1024, 2048, 1         # csrc/yaapt_long/yaapt_long.hip (held to it by the host test)
ARENA_FLOATS = 17                                                      # workspace floats per (utterance, frame) behind the resident layout


def gated(x, on=3 * yc.SR, off=yc.SR):
    """x with `on` samples kept, `off` samples zeroed, repeating"""
    t = torch.arange(x.shape[0]) % (on + off)
    return x * (t < on).to(x.dtype)


def _case(name, kind, make, n, **kw):
    return yc.Case(name, kind, make, n, math.ceil(n / 320), **kw)


CASES = [
    _case("tone_655361", "tone", lambda: yc.tone(655361), 655361, vuv=2048, nv=2048),
    _case("noisy1_655361", "noise", lambda: yc.noisy_tone(1, 655361), 655361),
    _case("gated2_660000", "noise", lambda: gated(yc.noisy_tone(2, 660000)), 660000),
    _case("jump_700000", "tone", lambda: yc.two_pitch(700000), 700000),
    _case("gated2_1310721", "noise", lambda: gated(yc.noisy_tone(2, 1310721)), 1310721),
    _case("noisy1_2621441", "noise", lambda: yc.noisy_tone(1, 2621441), 2621441, exact_only=True),
    _case("burst60_at8000_of655361", "burst", lambda: yc.tone(655361, 8000, 8060), 655361, nv=0, raises="RuntimeError"),
    _case("burst270_at8000_of655361", "burst", lambda: yc.tone(655361, 8000, 8270), 655361, nv=2, mean_nan=True),
]
FIXTURE_ONLY = ("noisy1_2621441",)      # no oracle-fed stage checks (and no oracle run on the CPU): the reference's track is the check


def by_name(name):
    return next(c for c in CASES if c.name == name)


def accepted():
    return [c for c in CASES if c.raises is None]


def raising():
    return [c for c in CASES if c.raises is not None]


def oracle_checked():
    """the accepted cases whose stages are also checked from the oracle fed with the device's intermediates (up to 4097 frames)"""
    return [c for c in accepted() if c.name not in FIXTURE_ONLY]


# a median window and a run of unvoiced frames across a chunk edge of 64: 130 frames; the tone stops inside frame 61 and comes back in
# frame 67, so frames 62 .. 66 carry no candidate (the compacted axis is shorter than the frame axis from there on), the 7-wide median of
# refine() at frames 61 .. 66 reads across frame 64, and the 5-wide one of spec_track across compacted index 64
def straddle():
    x = yc.tone(41281)
    x[61 * 320 + 100:66 * 320 + 200] = 0.0
    return x


STRADDLE = yc.Case("straddle64_41281", "tone", straddle, 41281, 130)


# ---- the chunk walk, restated ------------------------------------------------------------------------------------------------------------
def valid_chunk(chunk_frames):
    """the chunk the entry point runs with, None = refused"""
    if chunk_frames == 0:
        return DEFAULT_CHUNK
    if chunk_frames < CHUNK_STEP or chunk_frames > MAX_CHUNK or chunk_frames % CHUNK_STEP:
        return None
    return chunk_frames


def walk(T, CH):
    """path1_long over T frames in chunks of CH: per chunk (c0, n, staged frames, recursion frames, pred frames written); the path costs
    `pc` are carried from each chunk to the next in registers.  Frame 0 has no predecessor: no recursion step and no pred byte."""
    out = []
    for c0 in range(0, T, CH):
        n = min(CH, T - c0)
        staged = [t for t in range(c0 - HALO, c0 + n) if t >= 0]          # slot q = t - (c0 - HALO)
        steps = list(range(max(c0, 1), c0 + n))
        out.append(dict(c0=c0, n=n, staged=staged, steps=steps, pred=steps))
    return out


def walk_back(T, CH):
    """the back-trace: chunks in reverse; per chunk (c0, pred frames loaded, path frames written).  path[T - 1] is written before the
    walk; the step out of a chunk's first frame u writes path[u - 1], the last frame of the chunk before it: the state p is carried."""
    out = []
    for c0 in range((T - 1) // CH * CH, -1, -CH):
        n = min(CH, T - c0)
        us = list(range(c0 + n - 1, max(c0, 1) - 1, -1))
        out.append(dict(c0=c0, loaded=list(range(c0, c0 + n)), path=[u - 1 for u in us]))
    return out


def walk_means(T, CH):
    """yaapt_long_frame_means_kernel: per chunk the frames whose tails the four waves reduce into LDS, then walked by wave 0, which carries
    the previous mean and the prefetched head of frame k + 1 (frame c0 + n of the NEXT chunk at the edge)"""
    return [dict(c0=c0, frames=list(range(c0, min(c0 + CH, T))), prefetched=min(c0 + CH, T)) for c0 in range(0, T, CH)]


def lds_bytes(CH):
    """dynamic LDS of the two Viterbi kernels: staged float rows of CH + HALO slots, pred bytes of the chunk"""
    sp = CH + HALO
    return {"spec_post": 2 * 4 * sp * 4 + 4 * CH, "refine_dp": (2 * 6 + 1) * sp * 4 + 6 * CH}
