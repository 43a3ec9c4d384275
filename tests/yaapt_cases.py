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


def tone(n, on0=0, on1=None, gain=1.0, clip=None):
    """the harmonic tone, gated to [on0, on1), optionally amplified and clipped to +-clip"""
    t = np.arange(n, dtype=np.float64) / SR
    x = np.zeros(n, dtype=np.float64)
    for k in range(1, 6):
        x += 0.3 / k * np.sin(2 * np.pi * k * 120.0 * t)
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
                 refused=False, exact_only=False, underflows=False):
        self.name, self.kind, self.make, self.n, self.nframes = name, kind, make, n, nframes
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
            final, raised = oy.yaapt_one(case.wav(), OPTS, aux=aux), ""
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
        _JUDGED[case.name] = judge_oracle(oracle_run(case)[0], oy.Plan(case.n, OPTS), R)
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
