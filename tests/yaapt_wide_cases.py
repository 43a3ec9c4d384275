"""Input catalogue of the wide YAAPT tests (tests/test_yaapt_wide_host.py, tests/test_hip_yaapt_wide.py): option sets whose time-domain
frames overlap by MORE than the 128 samples of the resident kernels, the reference's own defaults among them.  sat_yaapt_long_f32 serves
them with its wide pair of kernels (csrc/yaapt_long/yaapt_long.hip); f0.track sends them there at every length.

time_track's frames are overlapping views of one buffer and crs_corr subtracts each frame's mean in place (yaapt.py:709-722, :589): with
n = tda_len, J = frame_jump and D = ceil(n / J) - 1, sample j of frame k has lost the means of the frames k - D .. k - 1 that cover it,
oldest first.  Samples n - (s + 1) J .. n - s J of a frame (its segment s) carry s earlier means: the tail (s = 0) none.

  set       options                                                n / J     ov   D  segments (s = D .. 0)   what it is there for
  defaults  {}                                                     560 / 160 400  3  80 / 160 / 160 / 160    the reference's defaults
  ov129     tda_frame_length 28.0625 on the anonymizer's options   449 / 320 129  1  129 / 320               the first overlap the resident
                                                                                                             forms refuse; a third head load
  d2_even   frame_space 10, tda_frame_length 30                    480 / 160 320  2  160 / 160 / 160         segment edges on frame edges
  d7        frame_length 40, frame_space 5, tda_frame_length 40    640 / 80  560  7  8 x 80                  the deepest plan accepted
  d8        frame_length 40, frame_space 4.5, tda_frame_length 40  640 / 72  568  8                          refused: D > 7

Signals (float64 synthesis rounded once, the generators of tests/yaapt_cases.py):
  mean70    the 120 Hz tone and a 70 Hz sinusoid of 0.4: 2.45 periods of 70 Hz per 560-sample frame, inside the 50 .. 1500 Hz pass band, so
            the frame means are NOT negligible against the samples and a wrong depth or order moves them far beyond the float64 bound
  gated     noisy_tone(2) gated 6000 samples on / 3000 off: runs of voiced and unvoiced frames
  noisy1, noisy5   the tone under white noise, seed 1 or 5.  The seeds: those under which no decision of the set hangs on the last bits
            (`near_ties` below; seed 1 under the defaults has a tie of two path costs at frame 104 that two units in the last place of one
            NCCF merit decide either way: seeds 5, 6 and 8 have none at either length)
  burst60   a 60-sample burst: frames above the NLFER threshold, none with a spectral candidate: the reference raises
  tone      the clean tone at 10 241 and 20 481 samples: 65 and 129 frames at the 10 ms hop, one past a chunk edge at chunk 64
  noisy5 at 327 681 samples: 2049 frames at the 10 ms hop, past the resident kernels' 2048
  rand3     1280 samples of torch.rand (tests/yaapt_cases.py `noise`), 8 frames: ONE frame with a spectral candidate, so `pitch_std` is the
            unbiased deviation of one value, NaN, and every NCCF merit with it: the NaN row of the ragged batch

The reference's own tracks: tests/golden/fx_f0_wide.npz (tests/golden/make_f0_wide_fixtures.py).  `frame_means_wide` restates the walk in
float32 (oracle.yaapt.frame_means is the one-deep case); the float64 references are tests/ref64_yaapt_wide.py."""
import math

import numpy as np
import torch

import yaapt_cases as yc
import yaapt_long_cases as ylc

SR = yc.SR
MAX_RESIDENT_OVERLAP = 128        # sat_yaapt_f32 / sat_yaapt_ragged_f32 (yaapt_check_plan)
MAX_DEPTH = 7                     # sat_yaapt_long_f32: YL_WIDE_DEPTH of csrc/yaapt_long/yaapt_long.hip


def depth(n, hop):
    return math.ceil(n / hop) - 1


def segments(n, hop):
    """lengths of the segments of a frame, s = D .. 0: segment s carries s earlier means"""
    D = depth(n, hop)
    return [n - D * hop] + [hop] * D


def mean70(n, sr=SR):
    t = np.arange(n, dtype=np.float64) / sr
    return (0.5 * yc.tone(n, sr=sr).double() + torch.from_numpy(0.4 * np.sin(2 * np.pi * 70.0 * t))).float()


SIGNALS = {
    "mean70": ("tone", lambda n: mean70(n)),
    "gated": ("noise", lambda n: ylc.gated(yc.noisy_tone(2, n), on=6000, off=3000)),
    "noisy1": ("noise", lambda n: yc.noisy_tone(1, n)),
    "noisy5": ("noise", lambda n: yc.noisy_tone(5, n)),
    "tone": ("tone", lambda n: yc.tone(n)),
    "burst60": ("burst", lambda n: yc.tone(n, 8000, 8060)),
    "rand3": ("noise", lambda n: yc.noise(3, n)),
}


class WideSet:
    """name, opts (handed to yaapt as they are), fields = the plan fields that put the set where it is (`ov` = tda_len - frame_jump, `D`,
    `segments`), signals = [(signal name, n)], raises = {signal_n: the reference's exception type}, refused = regex of the entry point's
    message"""

    def __init__(self, name, opts, fields, signals, raises=None, refused=None):
        self.name, self.opts, self.fields, self.refused = name, opts, dict(fields), refused
        raises = dict(raises or {})
        self.cases = []
        for sig, n in signals:
            from oracle import yaapt as oy
            kind, fn = SIGNALS[sig]
            self.cases.append(yc.Case(f"{name}/{sig}_{n}", kind, (lambda fn=fn, n=n: fn(n)), n, oy.Plan(n, opts).nframes, opts=opts,
                                      raises=raises.get(f"{sig}_{n}"), refused=refused is not None))

    def __repr__(self):
        return self.name


def _o(**kw):
    return {**yc.OPTS, **{k: float(v) for k, v in kw.items()}}


SETS = [
    WideSet("defaults", {}, dict(frame_size=560, tda_len=560, frame_jump=160, ov=400, D=3, segments=[80, 160, 160, 160]),
            [("mean70", 20480), ("gated", 20480), ("noisy5", 20480), ("burst60", 20480), ("tone", 10241), ("tone", 20481), ("noisy5", 327681),
             ("rand3", 1280)],
            raises={"burst60_20480": "RuntimeError"}),
    WideSet("ov129", _o(tda_frame_length=28.0625), dict(frame_size=560, tda_len=449, frame_jump=320, ov=129, D=1, segments=[129, 320]),
            [("mean70", 20480), ("noisy1", 20481)]),
    WideSet("d2_even", dict(frame_space=10.0, tda_frame_length=30.0), dict(tda_len=480, frame_jump=160, ov=320, D=2, segments=[160, 160, 160]),
            [("mean70", 20480), ("gated", 20480)]),
    WideSet("d7", dict(frame_length=40.0, frame_space=5.0, tda_frame_length=40.0),
            dict(frame_size=640, nframe_size=1280, tda_len=640, frame_jump=80, ov=560, D=7, segments=[80] * 8),
            [("mean70", 20480), ("noisy1", 10241)]),
    WideSet("d8", dict(frame_length=40.0, frame_space=4.5, tda_frame_length=40.0), dict(tda_len=640, frame_jump=72, ov=568, D=8),
            [("tone", 20480)], refused=r"a frame of 640 samples at a hop of 72 overlaps 8 earlier frames \(depth 8\), at most 7 are supported"),
]
MEAN70 = "defaults/mean70_20480"          # the case of the mutation test
CHUNK_EDGE = ("defaults/tone_10241", "defaults/tone_20481")     # 65 and 129 frames
BEYOND_RESIDENT = "defaults/noisy5_327681"                       # 2049 frames
NAN_ROW = "defaults/rand3_1280"                                  # pitch_std NaN


def wide_set(name):
    return next(s for s in SETS if s.name == name)


def cases():
    return [c for s in SETS for c in s.cases]


def by_name(name):
    return next(c for c in cases() if c.name == name)


def accepted():
    return [c for c in cases() if not c.refused and c.raises is None]


def raising():
    return [c for c in cases() if not c.refused and c.raises is not None]


def recorded():
    """what tests/golden/make_f0_wide_fixtures.py runs through the reference: every case of the accepted sets"""
    return [c for c in cases() if not c.refused]


# ---- the walk, restated in float32 -----------------------------------------------------------------------------------------------------
def frame_means_wide(filt, plan, means=None, mutate=None):
    """oracle.yaapt.frame_means for any depth: the de-meaned frames [T, n] as crs_corr sees them; the means are appended to `means`.
    Every subtraction is a float32 operation on the whole segment, in the reference's order: the oldest frame first.
    mutate, what the mutation test tries: None | "drop_oldest" (depth D - 1) | "newest_first" (the means taken newest first along the
    oldest-first walk: mean[k - 1] lands on the shortest span and mean[k - D] on the longest) | "reordered" (the right mean on the right
    span, but the newest subtracted first: the same real number, other roundings)"""
    T, n, hop = plan.tda_nframes, plan.tda_len, plan.frame_jump
    D = depth(n, hop)
    order = {None: range(D, 0, -1), "drop_oldest": range(D - 1, 0, -1), "newest_first": range(D, 0, -1), "reordered": range(1, D + 1)}[mutate]
    out = torch.empty(T, n)
    ms = []
    for k in range(T):
        v = filt[k * hop:k * hop + n].clone()
        for i in order:
            src = k - (D + 1 - i) if mutate == "newest_first" else k - i
            if k - i >= 0 and src >= 0:
                v[:n - i * hop] = v[:n - i * hop] - ms[src]
        m = torch.mean(v)
        ms.append(m)
        out[k] = v - m
    if means is not None:
        means.extend(ms)
    return out


# ---- the float32 oracle with the wide walk in place of its one-deep frame_means -----------------------------------------------------------
_ORACLE = {}


def oracle_run(case):
    """-> (aux, final track or None, name of the raised exception's type or "") of oracle.yaapt.yaapt_one with `frame_means_wide`, computed
    once.  aux also gets fmean1 / fmean2, the float32 frame means of the two signals"""
    from oracle import yaapt as oy
    if case.name not in _ORACLE:
        aux, got = {}, []

        def fm(filt, plan, means=None):
            ms = []
            out = frame_means_wide(filt, plan, means=ms)
            got.append(torch.stack(ms))
            return out

        keep, oy.frame_means = oy.frame_means, fm
        try:
            final, raised = oy.yaapt_one(case.wav(), case.opts, aux=aux), ""
        except Exception as e:                      # noqa: BLE001  (the type is the property under test)
            final, raised = None, type(e).__name__
        finally:
            oy.frame_means = keep
        if len(got) == 2:
            aux["fmean1"], aux["fmean2"] = got
        _ORACLE[case.name] = (aux, final, raised)
    return _ORACLE[case.name]


# ---- decisions that hang on the last bits ----------------------------------------------------------------------------------------------------
def near_ties(case, trials, ulps=2, seed=0):
    """frames of the float32 oracle's track that change when the NCCF merits and the energies are moved by up to `ulps` units in the last
    place at random (`trials` draws): refine + dynamic are run again on the perturbed values.  A float32 implementation that sums in another
    order than torch may land on either side at such a frame, so a track can be held against the reference's only where there is none
    -> {frame: draws that changed it}"""
    from oracle import yaapt as oy
    plan = oy.Plan(case.n, case.opts)
    aux, final, raised = oracle_run(case)
    assert raised == ""
    rng = np.random.default_rng(seed)

    def moved(t):
        a = t.numpy().copy()
        step = rng.integers(-ulps, ulps + 1, size=a.shape).astype(np.int32) * (np.isfinite(a) & (a != 0))
        return torch.from_numpy((a.view(np.int32) + step).view(np.float32))

    out = {}
    for _ in range(trials):
        en = moved(aux["energy"])
        rp, rm = oy.refine(aux["tp1"], moved(aux["tm1"]), aux["tp2"], moved(aux["tm2"]), aux["spec_pitch"].clone(), en, aux["vuv"], plan)
        f = oy.dynamic(rp, rm, en, plan)
        for k in torch.nonzero(~((f == final) | (torch.isnan(f) & torch.isnan(final)))).flatten().tolist():
            out[k] = out.get(k, 0) + 1
    return out
