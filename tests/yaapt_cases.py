"""Input catalogue of the YAAPT stage tests: deterministic utterances that sit on the kernels' edges, each with the
properties it is there for.

One wave per utterance walks the frames 64 at a time (`compact_frames`, `medfilt_par`, `mean_par`, the back-trace of
`path1_wave`), `yaapt_energy_norm_kernel` strides by 256, and `yaapt_spec_post_kernel` branches on the number `nv` of
frames with a spectral candidate: 0 (status 1, the reference raises), 1 (the unbiased deviation of one value is NaN and
`pitch_std` carries it into every NCCF merit), 2 (constant 150 Hz, no Viterbi), more.  The catalogue puts a frame count,
a count of voiced frames or `nv` on each of these edges and on the entry point's own limits of 4 and 2048 frames.

Synthesis is float64 rounded once to float32: the harmonic tone sum_{k=1..5} 0.3/k sin(2 pi k 120 t) at 16 kHz, gated to
[on0, on1).  With the project's options (frame_length 35, frame_space 20) nframes = ceil(n / 320).

The declared properties are asserted from the float32 oracle by tests/test_yaapt_cases_host.py on the CPU and again by
the GPU test from the oracle run it makes anyway, so a case that drifts off its edge fails loudly instead of silently
testing something else."""
import math

import numpy as np
import torch

OPTS = {"frame_length": 35.0, "frame_space": 20.0, "nccf_thresh1": 0.25, "tda_frame_length": 25.0}
SR = 16000
MIN_FRAMES, MAX_FRAMES = 4, 2048          # sat_yaapt_f32 accepts 4..2048 frames
DEFINITELY_UNVOICED = 0.1                 # nlfer_thresh2 (default): refine() discards the candidates of such a frame


def tone(n, on0=0, on1=None, gain=1.0, clip=None, f0=120.0, sr=SR):
    """the harmonic tone, gated to [on0, on1), optionally amplified and clipped to +-clip"""
    t = np.arange(n, dtype=np.float64) / sr
    x = np.zeros(n, dtype=np.float64)
    for k in range(1, 6):
        x += 0.3 / k * np.sin(2 * np.pi * k * f0 * t)
    gate = np.zeros(n, dtype=np.float64)
    gate[on0:n if on1 is None else on1] = 1.0
    x = x * gate * gain
    if clip is not None:
        x = np.clip(x, -clip, clip)
    return torch.from_numpy(x.astype(np.float32))


def noise(seed, n):
    """a row of `synthetic.rand_batch` (torch.rand in [0, 1): the reference README's smoke input)"""
    from satools_amd import synthetic
    return synthetic.rand_batch(seed, 1, n)[0]


class Case:
    """name, kind ('tone' | 'burst' | 'noise' | 'clip'), make() -> [n] float32, and the proven properties:
    nframes; vuv = frames above the NLFER threshold; nv = frames with a spectral candidate; std_nan = `pitch_std` is NaN;
    mean_nan = `mean_pitch` of dynamic() is NaN (the median-filtered best track has no positive frame);
    raises = the exception type of the reference (and of the oracle), device status 1;
    refused = outside the entry point's 4..2048 frames; exact_only = too long for the float64 stage references;
    underflows = the silence after the burst is long enough for the filters' tails to decay below float32's normal range:
    there the NCCF's sums of squares underflow, the float64 reference has no finite bound for a float32 result and lists
    the frames as `unbounded` (all of them definitely unvoiced, energy <= nlfer_thresh2); the cases without the flag have
    no such frame"""

    def __init__(self, name, kind, make, n, nframes, vuv=None, nv=None, std_nan=False, mean_nan=None, raises=None,
                 refused=False, exact_only=False, underflows=False, opts=None):
        self.name, self.kind, self.make, self.n, self.nframes = name, kind, make, n, nframes
        self.opts = OPTS if opts is None else opts          # the option set of the (case, set) pairs further down
        self.vuv, self.nv, self.std_nan, self.mean_nan = vuv, nv, std_nan, mean_nan
        self.raises, self.refused, self.exact_only, self.underflows = raises, refused, exact_only, underflows

    def wav(self):
        w = self.make()
        assert w.dtype == torch.float32 and w.shape == (self.n,)
        return w

    def __repr__(self):
        return self.name


def _tone(n, vuv, nv=None, **kw):
    return Case(f"tone_{n}", "tone", lambda: tone(n), n, math.ceil(n / 320), vuv=vuv, nv=vuv if nv is None else nv, **kw)


def _burst(length, at, n, vuv, nv, **kw):
    return Case(f"burst{length}_at{at}_of{n}", "burst", lambda: tone(n, at, at + length), n, math.ceil(n / 320), vuv=vuv, nv=nv, **kw)


CASES = [
    # ---- lane edges: frame count / voiced count / nv at 4, 63..65, 127..129, 255..257 -------------------------
    _tone(1280, 3, mean_nan=True),        # smallest accepted; spec_post's ta[0] = ta[2] with nf = 4
    _tone(1281, 4),
    _tone(1600, 4),
    _tone(20160, 62),                     # 63 frames
    _tone(20480, 63),                     # 64 frames
    _tone(20481, 64),                     # 65 frames, 64 voiced
    _tone(20800, 64),                     # 65 frames, nv on the lane edge
    _tone(21000, 65),                     # 66 frames, nv = 65
    _tone(40960, 127),                    # 128 frames
    _tone(41280, 128),                    # 129 frames
    _tone(41281, 129),                    # 130 frames
    _tone(81920, 255),                    # 256 frames: energy_norm's 256 stride
    _tone(82241, 256),                    # 258 frames, 256 voiced
    # ---- few voiced frames --------------------------------------------------------------------------------------
    _burst(260, 20220, 20480, 1, 1, std_nan=True, mean_nan=True),      # nv == 1: pitch_std NaN, every tm NaN
    _burst(280, 0, 20480, 2, 1, std_nan=True, mean_nan=True),          # the same at lane 0
    # nv <= 2: constant 150 Hz, pitch_std 7.5.  (260 samples at 0 or 8000 have two SHC peaks 4e-5 apart in one frame, inside
    # the float64 bound of the peak decision: 270 samples have the same properties and no such frame.)
    _burst(270, 0, 20480, 2, 2, mean_nan=True, underflows=True),
    _burst(270, 8000, 20480, 2, 2, mean_nan=True, underflows=True),
    _burst(320, 8000, 20480, 2, 2, mean_nan=True, underflows=True),
    _burst(640, 8000, 20480, 3, 2, mean_nan=True, underflows=True),
    _burst(960, 8000, 20480, 4, 4, mean_nan=True, underflows=True),    # smallest Viterbi
    _burst(300, 400, 1280, 2, 2, mean_nan=True),
    # the same branches with a tail too short to underflow: every frame of every stage has a finite bound
    _burst(260, 17280, 20480, 2, 2, mean_nan=True),
    _burst(320, 17600, 20480, 2, 2, mean_nan=True),
    _burst(640, 17600, 20480, 3, 2, mean_nan=True),
    _burst(960, 17600, 20480, 4, 4, mean_nan=True),
    # ---- frames above the NLFER threshold, no spectral candidate: the reference raises ------------------------------
    _burst(60, 8000, 20480, None, 0, raises="RuntimeError"),
    _burst(120, 8000, 20480, None, 0, raises="RuntimeError"),
    _burst(200, 8000, 20480, None, 0, raises="RuntimeError"),
    Case("rand2_1280", "noise", lambda: noise(2, 1280), 1280, 4, vuv=3, nv=0, raises="RuntimeError"),
    # ---- short noise rows: nv of 1 to 3 and a NaN mean_pitch in dynamic(); a clipped tone ----------------------------
    Case("rand0_1280", "noise", lambda: noise(0, 1280), 1280, 4, vuv=3, nv=1, std_nan=True, mean_nan=True),
    Case("rand3_1600", "noise", lambda: noise(3, 1600), 1600, 5, vuv=5, nv=2, mean_nan=True),
    Case("rand0_3200", "noise", lambda: noise(0, 3200), 3200, 10, vuv=8, nv=3, mean_nan=True),
    Case("clip40_20481", "clip", lambda: tone(20481, gain=40.0, clip=1.0), 20481, 65, vuv=64, nv=61, mean_nan=False),
    # ---- the entry point's limits --------------------------------------------------------------------------------
    Case("tone_960", "tone", lambda: tone(960), 960, 3, refused=True),
    Case("tone_655360", "tone", lambda: tone(655360), 655360, 2048, vuv=2047, nv=2047, exact_only=True),
    Case("tone_655361", "tone", lambda: tone(655361), 655361, 2049, refused=True),
]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def accepted():
    return [c for c in CASES if not c.refused and c.raises is None]


def raising():
    return [c for c in CASES if c.raises is not None]


def refused():
    return [c for c in CASES if c.refused]


def oracle_properties(aux):
    """the catalogue's properties from the aux dict of `oracle.yaapt.yaapt_one` (complete up to the stage that raised)"""
    out = {"nframes": int(aux["energy"].numel()), "vuv": int(aux["vuv"].sum()),
           "nv": int((aux["cand_pitch"][0] > 0).sum())}
    if "pitch_std" in aux:
        out["std_nan"] = bool(torch.isnan(aux["pitch_std"]))
    if "ref_pitch" in aux:
        best = aux["ref_pitch"][-2]
        out["mean_nan"] = not bool((best > 0).any())
    return out


def check_properties(case, aux):
    """assert what `case` declares; returns the measured properties"""
    got = oracle_properties(aux)
    assert got["nframes"] == case.nframes, (case, got)
    for key in ("vuv", "nv", "mean_nan"):
        want = getattr(case, key)
        if want is not None and key in got:
            assert got[key] == want, (case, key, got)
    if "std_nan" in got:
        assert got["std_nan"] == case.std_nan, (case, got)
    return got


# ---- the float32 oracle on the catalogue (shared by the CPU tests; run it with one torch thread) ----------------------
_ORACLE, _JUDGED = {}, {}


def oracle_run(case):
    """-> (aux, final track or None, name of the raised exception's type or "") of oracle.yaapt.yaapt_one, computed once"""
    from oracle import yaapt as oy
    if case.name not in _ORACLE:
        aux = {}
        try:
            final, raised = oy.yaapt_one(case.wav(), case.opts, aux=aux), ""
        except Exception as e:                      # noqa: BLE001  (the type is the property under test)
            final, raised = None, type(e).__name__
        _ORACLE[case.name] = (aux, final, raised)
    return _ORACLE[case.name]


def judge_oracle(aux, plan, R):
    """the oracle's intermediates of one utterance judged by the float64 references (tests/ref64_yaapt.py) the way the
    device's are: -> {stage: dict(ratio, exempt, wrong)}"""
    import ref64_yaapt as r64
    from oracle import yaapt as oy
    filt, filt2 = aux["filt"].numpy(), aux["filt2"].numpy()
    out = {"vuv": r64.judge_vuv(filt, aux["energy"].numpy(), aux["vuv"].numpy(), plan, R),
           "cand": r64.judge_cand(filt2, aux["vuv"].numpy(), aux["cand_pitch"].numpy(), aux["cand_merit"].numpy(), plan, R)}
    sp, pstd = aux["spec_pitch"].numpy(), float(aux["pitch_std"])
    for sig, x, tp, tm in ((1, aux["filt"], aux["tp1"], aux["tm1"]), (2, aux["filt2"], aux["tp2"], aux["tm2"])):
        means = []
        oy.frame_means(x, plan, means=means)
        means = np.array([float(m) for m in means], np.float32)
        out[f"fmean{sig}"] = r64.judge_fmean(x.numpy(), means, plan, R)
        out[f"nccf{sig}"] = r64.judge_nccf(x.numpy(), means, sp, pstd, tp[0].numpy(), tm[0].numpy(), plan, R)
    return out


def judged_oracle(case, R):
    from oracle import yaapt as oy
    if case.name not in _JUDGED:
        _JUDGED[case.name] = judge_oracle(oracle_run(case)[0], oy.Plan(case.n, case.opts), R)
    return _JUDGED[case.name]


def exempt_frames(res):
    """frames some stage exempts -> {stage: frames} (`<stage>/unbounded`: the NCCF frames without a finite bound)"""
    out = {stage: r["exempt"] for stage, r in res.items() if r.get("exempt")}
    out.update({stage + "/unbounded": r["unbounded"] for stage, r in res.items() if r.get("unbounded")})
    return out


def assert_exempt_cap(case, res, energy):
    """the condition on the catalogue: no exempt frame on the gated-tone cases, at most 1 % of the frames (of any one
    stage) on the noise and clipped cases.  Frames without a finite bound are allowed on the cases that declare
    `underflows` only, and only where `energy` (the implementation's own) says definitely unvoiced."""
    ex = exempt_frames(res)
    cap = 0 if case.kind in ("tone", "burst") else int(0.01 * case.nframes)
    unbounded = set()
    for stage, frames in ex.items():
        if stage.endswith("/unbounded"):
            unbounded.update(frames)
        else:
            assert len(frames) <= cap, (case, stage, frames, f"cap {cap}")
    assert bool(unbounded) == case.underflows, (case, sorted(unbounded))
    for k in unbounded:
        assert float(energy[k]) <= DEFINITELY_UNVOICED, (case, k, float(energy[k]))
    return ex


# ======================================================================================================================
# OPTION SETS.  Every case above runs under OPTS, i.e. ONE plan (frame_size 560, frame_jump 320, tda_len 400 with an overlap of 80,
# nharm 3, median 7, max_shc 256, wl 21, bins 60..205, every scalar at one value).  The table below moves the plan: each set names
# the edge it is there for and the plan fields that put it there (asserted from oracle.yaapt.Plan by the host test, so a typo cannot
# move a set off its edge), and carries two or three signals of its own: a tone whose frame count sits on a lane edge for the set's
# jump, a clipped or noisy one, and for the limit sets a burst with few voiced frames.
#   accepted   the reference runs (tests/golden/fx_f0_options.npz holds its tracks), the device must agree stage by stage
#   wiring     one scalar option changed against OPTS; `observe` names the oracle intermediate (or the final track) that changes on
#              the set's signal, so that a kernel which ignores the option fails
#   refused    outside the entry point's region of plans: `refused` is the message of the requirement that refuses it
#   status 2   every frame's NCCF window is empty (N = tda_len - lag_max <= 0): the reference asserts, the device reports status 2
# A case of a set is named "<set>/<signal>".
# ======================================================================================================================
def two_level(n, sr=SR):
    """the tone, its second half at 0.3 of the level: frames with a normalised energy between nlfer_thresh2 and nlfer_thresh1"""
    return torch.cat((tone(n, sr=sr)[:n // 2], 0.3 * tone(n, sr=sr)[n // 2:]))


def two_pitch(n, sr=SR):
    """150 Hz, then 100 Hz: spectral candidates that disagree from frame to frame (the Viterbi costs decide).  (120 Hz then 200 Hz
    widens `pitch_std` to 40 Hz and with it the lag window of frame 0, most of which is padding: its NCCF is flat to within the
    float64 bound, an exempt frame)"""
    return torch.cat((tone(n, f0=150.0, sr=sr)[:n // 2], tone(n, f0=100.0, sr=sr)[n // 2:]))


def noisy_tone(seed, n):
    """the tone under white noise: NCCF frames whose first local peak is not the largest within nccf_pwidth (nccf_thresh2 decides),
    and outliers in the best track that each median width smooths differently (a clean tone's track is constant: any width passes)"""
    return 0.5 * tone(n) + 0.3 * (2.0 * noise(seed, n) - 1.0)


SIGNALS = {
    "tone": ("tone", lambda n, sr: tone(n, sr=sr)),
    "tone200": ("tone", lambda n, sr: tone(n, f0=200.0, sr=sr)),
    "tone170": ("tone", lambda n, sr: tone(n, f0=170.0, sr=sr)),
    "clip40": ("clip", lambda n, sr: tone(n, gain=40.0, clip=1.0, sr=sr)),
    "clip100": ("clip", lambda n, sr: tone(n, gain=100.0, clip=1.0, sr=sr)),
    "level": ("tone", two_level),
    "jump": ("tone", two_pitch),
    "noisy1": ("noise", lambda n, sr: noisy_tone(1, n)),
    "noisy2": ("noise", lambda n, sr: noisy_tone(2, n)),
    # (the seeds: those whose float32 decisions all clear the float64 bounds under their set, tests/test_yaapt_cases_host.py)
    "noisy4": ("noise", lambda n, sr: noisy_tone(4, n)),
    "noisy9": ("noise", lambda n, sr: noisy_tone(9, n)),
    "rand0": ("noise", lambda n, sr: noise(0, n)),
}


class OptionSet:
    """name, opts (handed to yaapt as they are), why = the edge in words, fields = the plan fields that put the set there (`ov` =
    tda_len - frame_jump), signals = [(signal name, n) | ("burst", length, at, n)]; refused = regex of the entry point's message (its
    one case is what the refusal is tried on); wiring = (key, observe); raises = {signal: exception type}"""

    def __init__(self, name, opts, why, fields=None, signals=(), refused=None, wiring=None, raises=None):
        self.name, self.opts, self.why, self.fields = name, opts, why, dict(fields or {})
        self.refused, self.wiring = refused, wiring
        self.raises = dict(raises or {})           # signal name -> the oracle's exception type (the reference's: see the fixture)
        self.cases = [self._case(s) for s in signals]

    def _case(self, s):
        from oracle import yaapt as oy
        sr = float(self.opts.get("sr", SR))
        if s[0] == "burst":
            _, length, at, n = s
            name, kind, make = f"burst{length}_at{at}_of{n}", "burst", (lambda: tone(n, at, at + length, sr=sr))
        else:
            sig, n = s
            kind, fn = SIGNALS[sig]
            name, make = f"{sig}_{n}", (lambda: fn(n, sr))
        return Case(f"{self.name}/{name}", kind, make, n, oy.Plan(n, self.opts).nframes, opts=self.opts, raises=self.raises.get(name),
                    refused=self.refused is not None)

    def __repr__(self):
        return self.name


def _o(**kw):
    return {**OPTS, **{k: float(v) for k, v in kw.items()}}


ALL_SCALARS = dict(nlfer_thresh1=0.7, nlfer_thresh2=0.15, shc_thresh1=4.5, shc_thresh2=1.3, f0_double=160.0, f0_half=140.0, dp5_k1=9.0,
                   nccf_thresh1=0.3, nccf_thresh2=0.85, merit_boost=0.25, merit_pivot=0.95, merit_extra=0.45, dp_w1=0.2, dp_w2=0.45,
                   dp_w3=0.15, dp_w4=0.8, spec_pitch_min_std=0.06)

OPTION_SETS = [
    # ---- the plan's extents --------------------------------------------------------------------------------------------
    OptionSet("jump512_ov128", _o(frame_length=40, frame_space=32, tda_frame_length=40),
              "nframe_size = 1280 = 5 * 256 (the whole magnitude hand-over and kaiser loop), overlap 128 (the second head load of "
              "yaapt_frame_means_kernel in full)", dict(frame_size=640, nframe_size=1280, frame_jump=512, tda_len=640, ov=128),
              [("tone", 64 * 512 + 1), ("clip40", 63 * 512), ("burst", 1536, 28160, 63 * 512)]),
    OptionSet("tda1024", _o(frame_length=40, frame_space=56, tda_frame_length=64),
              "tda_len = 1024: the whole of d[1024] / phi[1024]; frame_space > frame_length, at lengths where the reference's zero "
              "extension is not negative and the tda frames equal the analysis frames (n mod 896 in 384..640)",
              dict(frame_size=640, nframe_size=1280, frame_jump=896, tda_len=1024, ov=128),
              [("tone", 64 * 896 + 512), ("clip40", 62 * 896 + 384), ("burst", 2688, 12288, 19 * 896 + 640)]),
    OptionSet("ov1", _o(tda_frame_length=20.0625), "overlap 1: one head sample per frame", dict(tda_len=321, frame_jump=320, ov=1),
              [("tone", 20481), ("clip40", 20160)]),
    OptionSet("short", _o(frame_length=20, frame_space=10, tda_frame_length=17), "short frames, overlap 112, 128 / 129 frames",
              dict(frame_size=320, nframe_size=640, frame_jump=160, tda_len=272, ov=112), [("tone200", 20480), ("clip40", 20481)]),
    OptionSet("sr8000", _o(sr=8000, f0_max=140), "8 kHz: every length halves, delta halves (wl 41, pk_center 26)",
              dict(frame_size=280, frame_jump=160, tda_len=200, wl=41, pk_center=26, nframe_size=560),
              [("tone", 64 * 160), ("clip40", 64 * 160 + 1)]),
    OptionSet("sr22050", _o(sr=22050, frame_length=25, frame_space=15, tda_frame_length=20),
              "22.05 kHz: odd frame size and jump, the unaligned prefilter path by construction",
              dict(frame_size=551, frame_jump=330, tda_len=441, ov=111, pad=275), [("tone", 64 * 330 + 1), ("clip100", 63 * 330)]),
    # ---- harmonics, median, ranges ---------------------------------------------------------------------------------------
    OptionSet("nharm1", _o(shc_numharms=1), "one harmonic product", dict(nharm=1), [("tone", 20481), ("clip40", 20160)]),
    OptionSet("nharm4_f0max350", _o(shc_numharms=4, f0_max=350), "four harmonics, a narrower SHC range",
              dict(nharm=4, max_shc=230, pk_max_lag=192), [("tone", 20480), ("clip40", 20481)]),
    OptionSet("nharm6_f0max250", _o(shc_numharms=6, f0_max=250),
              "the largest harmonic count the 1280-float magnitude window admits on signals the reference runs on: "
              "max_shc * (nharm + 1) + wl = 179 * 7 + 21 = 1274 <= 1280 (7 harmonics need f0_max <= 206, where the reference "
              "fails on the catalogue's signals: see nharm7_f0max200)", dict(nharm=6, max_shc=179),
              [("tone", 20481), ("clip40", 20160), ("burst", 960, 17600, 20480)]),
    OptionSet("median1", _o(median_value=1), "median width 1 (and 1 in spec_track)", dict(median_value=1), [("tone", 20481), ("clip40", 20160), ("noisy4", 20481)]),
    OptionSet("median3", _o(median_value=3), "median width 3 (1 in spec_track)", dict(median_value=3), [("tone", 20480), ("noisy1", 20481)]),
    OptionSet("median5", _o(median_value=5), "median width 5 (3 in spec_track)", dict(median_value=5), [("tone", 20160), ("noisy9", 20481)]),
    OptionSet("f0_50_300", _o(f0_min=50, f0_max=300), "NLFER bins 50..154, min_shc 26", dict(nl_lo=50, nl_hi=154, min_shc=26),
              [("tone", 20481), ("clip40", 20160)]),
    OptionSet("f0min80_pw30_win60", _o(f0_min=80, shc_pwidth=30, shc_window=60), "SHC window 31, peak half-width 8, first lag 32",
              dict(wl=31, half_wl=15, pk_center=8, pk_min_lag=32), [("tone", 20481), ("clip40", 20160)]),
    OptionSet("nccf_pwidth9", _o(nccf_pwidth=9), "NCCF peak half-width 4", dict(nccf_center=4), [("tone", 20481), ("noisy2", 20481)]),
    OptionSet("bandpass", _o(bp_low=80, bp_high=1000), "other biquad coefficients", {}, [("tone200", 20481), ("clip40", 20160)]),
    OptionSet("all_scalars", {**OPTS, **ALL_SCALARS}, "every threshold and weight off its default at once", {},
              [("tone", 20481), ("clip40", 20160), ("jump", 20481)]),
    # ---- wiring: one scalar changed against OPTS, on a signal where the oracle's output changes ------------------------
    OptionSet("w_nlfer_thresh1", _o(nlfer_thresh1=0.5), "wiring", {}, [("tone", 20481)], wiring=("nlfer_thresh1", "vuv")),
    OptionSet("w_nlfer_thresh2", _o(nlfer_thresh2=0.5), "wiring", {}, [("level", 20481)], wiring=("nlfer_thresh2", "final")),
    OptionSet("w_shc_thresh1", _o(shc_thresh1=3.0), "wiring", {}, [("clip40", 20481)], wiring=("shc_thresh1", "final")),
    OptionSet("w_shc_thresh2", _o(shc_thresh2=2.5), "wiring", {}, [("tone", 20481)], wiring=("shc_thresh2", "cand_merit")),
    OptionSet("w_f0_double", _o(f0_double=200.0), "wiring", {}, [("tone170", 20481)], wiring=("f0_double", "cand_pitch")),
    OptionSet("w_f0_half", _o(f0_half=100.0), "wiring", {}, [("tone", 20481)], wiring=("f0_half", "cand_pitch")),
    OptionSet("w_dp5_k1", _o(dp5_k1=1000.0), "wiring", {},
              [("jump", 20481)], wiring=("dp5_k1", "final")),
    OptionSet("w_nccf_thresh1", _o(nccf_thresh1=0.6), "wiring", {}, [("clip40", 20481)], wiring=("nccf_thresh1", "final")),
    OptionSet("w_nccf_thresh2", _o(nccf_thresh2=0.25), "wiring", {}, [("noisy1", 20481)], wiring=("nccf_thresh2", "tp1+tp2")),
    OptionSet("w_merit_boost", _o(merit_boost=0.3), "wiring", {}, [("clip40", 20481)], wiring=("merit_boost", "final")),
    # merit_pivot fills rows of refine() at frames with energy <= nlfer_thresh2; their pitch is 0 in every row but the spectral one, which
    # costs ~1 there, so the FINAL track does not move with it on any signal tried (level steps, fades, dips around the threshold, noise,
    # pivots from 0 to 3): the device test compares the refined rows themselves (workspace view "refined")
    OptionSet("w_merit_pivot", _o(merit_pivot=0.9), "wiring", {}, [("burst", 960, 17600, 20480)], wiring=("merit_pivot", "ref_merit")),
    OptionSet("w_merit_extra", _o(merit_extra=0.6), "wiring", {}, [("tone", 20481)], wiring=("merit_extra", "cand_merit")),
    OptionSet("w_dp_w1", _o(dp_w1=5.0), "wiring", {}, [("jump", 20481)], wiring=("dp_w1", "final")),
    OptionSet("w_dp_w2", _o(dp_w2=0.05), "wiring", {}, [("clip40", 20481)], wiring=("dp_w2", "final")),
    OptionSet("w_dp_w3", _o(dp_w3=0.6), "wiring", {}, [("clip40", 20481)], wiring=("dp_w3", "final")),
    OptionSet("w_dp_w4", _o(dp_w4=0.3), "wiring", {}, [("clip40", 20481)], wiring=("dp_w4", "final")),
    OptionSet("w_spec_pitch_min_std", _o(spec_pitch_min_std=0.2), "wiring", {}, [("clip40", 20481)],
              wiring=("spec_pitch_min_std", "final")),
    # ---- the reference raises: the device must end the same way --------------------------------------------------------
    OptionSet("status2", dict(frame_length=10.0, frame_space=5.0, tda_frame_length=12.0),
              "tda_len 192: N = tda_len - lag_max <= 0 in the frames of a 120 Hz tone (status 2); a 200 Hz tone has none",
              dict(tda_len=192, frame_jump=80, frame_size=160), [("tone", 20480), ("tone200", 20480)], raises={"tone_20480": "AssertionError"}),
    OptionSet("nharm7_f0max200", _o(shc_numharms=7, f0_max=200),
              "seven harmonics fit the magnitude window below f0_max = 206 only; the SHC of the tone then peaks at its octave, above "
              "f0_max by more than two deviations: lag_max < lag_min, the reference fails in crs_corr (status 3)", dict(nharm=7, max_shc=153),
              [("tone", 20480)], raises={"tone_20480": "RuntimeError"}),
    # ---- refused ---------------------------------------------------------------------------------------------------------
    OptionSet("reference_defaults", {}, "the reference's own defaults: overlap 400 > 128", dict(tda_len=560, frame_jump=160), signals=[("tone", 20480)],
              refused="tda_frame_length / frame_space combination not supported"),
    OptionSet("fft4096", _o(fft_length=4096), "", {}, signals=[("tone", 20480)], refused=r"fft_length 4096 not supported \(8192 only\)"),
    OptionSet("maxpeaks5", _o(shc_maxpeaks=5), "", {}, signals=[("tone", 20480)], refused="shc_maxpeaks/nccf_maxcands must be 4/3"),
    OptionSet("maxcands4", _o(nccf_maxcands=4), "", {}, signals=[("tone", 20480)], refused="shc_maxpeaks/nccf_maxcands must be 4/3"),
    OptionSet("median9", _o(median_value=9), "", {}, signals=[("tone", 20480)], refused="median_value must be odd <= 7"),
    OptionSet("median4", _o(median_value=4), "", {}, signals=[("tone", 20480)], refused="median_value must be odd <= 7"),
    OptionSet("frame41", _o(frame_length=41), "nframe_size 1312 > 1280", dict(nframe_size=1312), signals=[("tone", 20480)], refused="frame_length too long for the spectral kernel"),
    OptionSet("nharm8", _o(shc_numharms=8), "", {}, signals=[("tone", 20480)], refused="shc_numharms out of range"),
    OptionSet("tda_le_space", _o(tda_frame_length=20), "tda_len == frame_jump", dict(tda_len=320, frame_jump=320), signals=[("tone", 20480)],
              refused="tda_frame_length / frame_space combination not supported"),
    OptionSet("space_gt_frame", _o(frame_space=56, tda_frame_length=64),
              "frame_space > frame_length at a length where the last spectral frame ends inside the padded signal: the reference fails "
              "on a negative zero extension", dict(frame_jump=896, tda_len=1024), [("tone", 20480)], refused="frame_space too long for frame_length",
              raises={"tone_20480": "RuntimeError"}),
]


def option_set(name):
    return next(s for s in OPTION_SETS if s.name == name)


def accepted_sets():
    """the sets the device accepts and the reference runs on (the wiring sets among them)"""
    return [s for s in OPTION_SETS if not s.refused and not s.raises]


def raising_sets():
    """accepted by the entry point, but the reference raises on (some of) their signals: a status word must say so"""
    return [s for s in OPTION_SETS if not s.refused and s.raises]


def refused_sets():
    return [s for s in OPTION_SETS if s.refused]


def option_cases():
    """every (case, set) pair the device must agree with the reference on, stage by stage"""
    return [c for s in OPTION_SETS if not s.refused for c in s.cases if c.raises is None]


def recorded_cases():
    """what tests/golden/make_f0_edge_fixtures.py runs through the reference: every pair of the sets the entry point accepts, and
    the refused set on which the reference has a word of its own (the other refusals are limits of the device alone)"""
    return [c for s in OPTION_SETS if not s.refused or s.raises for c in s.cases]


def any_order(plan):
    """rounding counts of a float32 implementation that sums in any order (what the float32 oracle, i.e. torch, is judged with):
    tests/test_ref64_yaapt.py's ANY_ORDER with the frame-mean counts taken from the plan instead of the 400 samples of OPTS"""
    import ref64_yaapt as r64
    return r64.Roundings(cmul=3.25, hyp=4, nl_sum=lambda n: n, en_mean=lambda n: n, sp_mean=lambda n: n + 1, shc_sum=lambda n: n,
                         shc_avg=lambda n: n, fm_head=lambda n: plan.tda_len + 1, fm_tail=lambda n: plan.tda_len,
                         dot=lambda n: n + 1, pw=lambda n: n + 1)
