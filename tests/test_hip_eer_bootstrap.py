"""The bootstrap replicates of the empirical EER on the device (csrc/stats/eer_bootstrap.hip, include/satools_hip_stats.h) against the
restatement of tests/ref64_eer.py.  The device work is integers and a replicate is a function of (seed, its number) alone, so every
comparison here is EQUALITY of the two int32 counts of every replicate (torch.equal) — there is no tolerance in this file — and the
float64 replicate EERs, the same division of the same integers on both sides, are equal to the last bit.

Shapes: the smallest at which the kernel can go wrong — one trial a side, one side of one, very unequal sides, the lane / wave / block
edges of the counting sweep, the Philox word tail (n = 1, 2, 3 mod 4), heavy ties (K = 3), separated sets (EER 0 and 1), both sides of the
switch between the kernel's two forms (a wave owns a replicate up to n_tar + n_non = 4096, a block of 256 threads above), the
VoxCeleb1-O size and the supported maximum; m runs over 1, 2, 63, 64, 65, 257 (grid edges of both forms: four replicates a block in the
wave form, one in the block form).  Also: independence of the launch split, the stream and the seed; eer_interval; every refusal of the
entry point; and the red-zone table ROWS of this entry point (tests/moat.py), which tests/test_eer_host.py holds against the header.
Needs a real MI355X: run with `-m gpu`."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import ref64_eer
from moat import Buf, run_case

DEV = "cuda"
I32 = torch.int32
ENTRY = "sat_eer_bootstrap_i32"
FAMILIES = ["eer_bootstrap_kernel"]           # every SAT_LAUNCH_CHECK string of csrc/stats/ (tests/test_eer_host.py holds this against the sources)
WAVE_MAX = 4096                               # EB_WAVE_MAX of the kernel: n_tar + n_non up to which a wave owns a replicate
MAX_SIDE = 1 << 20                            # SAT_EER_BOOTSTRAP_MAX_SIDE

# (n_tar, n_non, kind of scores, m)
TABLE = [
    (1, 1, "overlap", 65),                    # smallest size; one Philox call a side
    (1, 5, "overlap", 64), (5, 1, "overlap", 63),                                   # one side of size one
    (3, 1000, "overlap", 257), (1000, 3, "overlap", 2),                             # very unequal sides
    (63, 65, "overlap", 1), (64, 64, "overlap", 65), (255, 257, "overlap", 63), (256, 256, "overlap", 64), (1023, 1025, "overlap", 257),      # lane, wave and block edges
    (4097, 4095, "overlap", 65),              # past one sweep of a block (1024 Philox calls a sweep at 4096 a side: eight per thread)
    (9, 6, "overlap", 64), (10, 7, "overlap", 2), (11, 8, "overlap", 63), (12, 12, "overlap", 1),                                             # n = 1, 2, 3, 0 mod 4
    (37, 41, "ties3", 257), (2500, 2400, "ties3", 63),                              # three distinct values, K = 3: both forms
    (50, 70, "above", 64), (3000, 2000, "above", 2),                                # all targets above all non-targets: every replicate (0, .), EER 0
    (50, 70, "below", 65), (3000, 2000, "below", 1),                                # all below: EER 1
    (2048, 2048, "overlap", 257), (4000, 96, "overlap", 64),                        # n_tar + n_non = 4096: the last size of the wave form
    (2049, 2048, "overlap", 257), (4000, 97, "overlap", 64),                        # 4097: the first of the block form
    (18860, 18860, "overlap", 64),            # VoxCeleb1-O size
    (MAX_SIDE, MAX_SIDE - 3, "overlap", 4),   # the supported maximum
]
assert {t[3] for t in TABLE} >= {1, 2, 63, 64, 65, 257}
assert any(a + b == WAVE_MAX for a, b, _, _ in TABLE) and any(a + b == WAVE_MAX + 1 for a, b, _, _ in TABLE)


def _sat():
    import satools_amd  # noqa: F401
    from satools_amd import _lib, asv_eval, ops
    return _lib, ops, asv_eval


@functools.lru_cache(maxsize=None)
def scores(n_tar, n_non, kind):
    """-> (sorted targets, sorted non-targets) float64"""
    g = np.random.default_rng(n_tar * 7919 + n_non)
    if kind == "overlap":
        tar, non = g.normal(1, 1, n_tar), g.normal(-1, 1, n_non)
    elif kind == "ties3":
        tar, non = g.integers(0, 3, n_tar).astype(np.float64), g.integers(0, 3, n_non).astype(np.float64)
        tar[0], non[0] = 2.0, 0.0
        if n_tar > 1:
            tar[1] = 1.0
    elif kind == "above":
        tar, non = 5 + g.random(n_tar), g.random(n_non)
    else:
        tar, non = g.random(n_tar), 5 + g.random(n_non)
    return np.sort(tar), np.sort(non)


@functools.lru_cache(maxsize=None)
def want(n_tar, n_non, kind, m, seed=0, first=0):
    """the restatement's replicates, computed once per case and shared -> (miss_at, fa_before) int32 CPU tensors (never modified)"""
    miss, fa = ref64_eer.replicates(*scores(n_tar, n_non, kind), first, m, seed)
    return torch.from_numpy(miss).to(I32), torch.from_numpy(fa).to(I32)


def cuts(n_tar, n_non, kind):
    return _sat()[2].eer_cuts(*scores(n_tar, n_non, kind))


def _id(c):
    return "x".join(str(v) for v in c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_replicates_equal_the_restatement(case):
    n_tar, n_non, kind, m = case
    _lib, ops, asv_eval = _sat()
    ct, cn = cuts(n_tar, n_non, kind)
    if kind == "ties3":
        assert len(ct) == 4
    miss, fa = ops.eer_bootstrap(ct, cn, n_tar, n_non, m, seed=0, device=DEV)
    assert miss.dtype == fa.dtype == I32 and miss.is_cuda and tuple(miss.shape) == tuple(fa.shape) == (m,)
    wm, wf = want(n_tar, n_non, kind, m)
    assert torch.equal(miss.cpu(), wm) and torch.equal(fa.cpu(), wf), (case, miss.cpu()[:8], wm[:8], fa.cpu()[:8], wf[:8])
    assert _lib.lib().sat_last_dispatch_name().decode().split("<")[0].strip() == "eer_bootstrap_kernel"
    if kind == "above":
        assert not bool(miss.any())                                               # EER 0 in every replicate
    if kind == "below":
        assert bool((miss == n_tar).all()) and bool((fa == n_non).all())          # EER 1


@pytest.mark.gpu
@pytest.mark.parametrize("n_tar, n_non", [(200, 300), (3000, 2500)], ids=["wave", "block"])
def test_replicates_do_not_depend_on_the_launch(n_tar, n_non):
    _lib, ops, _ = _sat()
    ct, cn = cuts(n_tar, n_non, "overlap")
    dct, dcn = torch.from_numpy(ct).to(DEV), torch.from_numpy(cn).to(DEV)          # (tables already on the device are taken as they are)
    whole = ops.eer_bootstrap(dct, dcn, n_tar, n_non, 5, seed=11)
    a = ops.eer_bootstrap(ct, cn, n_tar, n_non, 2, seed=11, first_replicate=0, device=DEV)
    b = ops.eer_bootstrap(ct, cn, n_tar, n_non, 3, seed=11, first_replicate=2, device=DEV)
    for i in range(2):
        assert torch.equal(whole[i], torch.cat([a[i], b[i]]))
        assert torch.equal(whole[i].cpu(), want(n_tar, n_non, "overlap", 5, 11)[i])
    far = ops.eer_bootstrap(ct, cn, n_tar, n_non, 3, seed=11, first_replicate=2 ** 31 - 4, device=DEV)      # the last replicate numbers there are
    for i in range(2):
        assert torch.equal(far[i].cpu(), want(n_tar, n_non, "overlap", 3, 11, 2 ** 31 - 4)[i])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = ops.eer_bootstrap(dct, dcn, n_tar, n_non, 5, seed=11)
    side.synchronize()
    again = ops.eer_bootstrap(ct, cn, n_tar, n_non, 5, seed=11, device=DEV)
    other = ops.eer_bootstrap(ct, cn, n_tar, n_non, 5, seed=12, device=DEV)
    wide = ops.eer_bootstrap(ct, cn, n_tar, n_non, 5, seed=11 + (1 << 32), device=DEV)      # the upper key word counts
    for i in range(2):
        assert torch.equal(s[i], whole[i]) and torch.equal(again[i], whole[i])
    assert not (torch.equal(other[0], whole[0]) and torch.equal(other[1], whole[1]))
    assert not (torch.equal(wide[0], whole[0]) and torch.equal(wide[1], whole[1]))
    assert torch.equal(wide[0].cpu(), want(n_tar, n_non, "overlap", 5, 11 + (1 << 32))[0])


@pytest.mark.gpu
def test_eer_interval_equals_the_interval_of_the_restatements_replicates():
    """N(1, 1) against N(-1, 1), 2 000 a side, 2 000 replicates: the replicates are exact, so the percentile interval is too"""
    _, _, asv_eval = _sat()
    g = np.random.default_rng(2024)
    tar, non = g.normal(1, 1, 2000), g.normal(-1, 1, 2000)
    eer, lower, upper, reps = asv_eval.eer_interval(tar, non, m=2000, ci=0.95, seed=5, device=DEV)
    miss, fa = ref64_eer.replicates(np.sort(tar), np.sort(non), 0, 2000, 5)
    w = np.minimum(miss.astype(np.float64) / 2000, fa.astype(np.float64) / 2000)
    assert reps.dtype == np.float64 and reps.tobytes() == w.tobytes()
    lo, up = np.percentile(w, [2.5, 97.5])
    assert (lower, upper) == (float(lo), float(up)) and 0.0 <= lower <= upper <= 1.0
    m0, f0 = ref64_eer.eer_counts(np.sort(tar), np.sort(non), np.arange(2000), np.arange(2000))
    assert eer == min(m0 / 2000, f0 / 2000) == asv_eval.empirical_eer(tar, non)[0]
    print(f"eer_interval: EER {eer:.4f}, 95 % interval {lower:.4f} .. {upper:.4f}")
    m, _, _ = asv_eval.score_metrics(tar, non, eer_ci=dict(m=64, ci=0.95, seed=5, device=DEV))
    try:
        import feerci  # noqa: F401
    except ImportError:
        assert 0.0 <= m["eer_lower"] <= m["eer_upper"] <= 100.0 and 0.0 <= m["eer"] <= 100.0


@pytest.mark.gpu
def test_entry_point_refuses_bad_arguments_and_launches_nothing():
    _lib, _, _ = _sat()
    L = _lib.lib()
    n_tar, n_non, m = 5, 7, 3
    ct, cn = cuts(n_tar, n_non, "overlap")
    K = len(ct) - 1
    dct, dcn = torch.from_numpy(ct).to(DEV), torch.from_numpy(cn).to(DEV)
    miss, fa = torch.full((m,), -7, dtype=I32, device=DEV), torch.full((m,), -9, dtype=I32, device=DEV)
    P = lambda t: t.data_ptr()
    good = dict(ct=P(dct), cn=P(dcn), K=K, n_tar=n_tar, n_non=n_non, first=0, m=m, miss=P(miss), fa=P(fa))
    bad = {
        "null cut_tar": dict(ct=None), "null cut_non": dict(cn=None), "null miss_at": dict(miss=None), "null fa_before": dict(fa=None),
        "n_tar = 0": dict(n_tar=0), "n_non = 0": dict(n_non=0), "n_tar < 0": dict(n_tar=-1), "m = 0": dict(m=0), "m < 0": dict(m=-2),
        "K = 0": dict(K=0), "K above n_tar + n_non": dict(K=n_tar + n_non + 1),
        "first < 0": dict(first=-1), "first + m past int32": dict(first=2 ** 31 - 3), "first at int32 max": dict(first=2 ** 31 - 1),
        "n_tar above the maximum": dict(n_tar=MAX_SIDE + 1), "n_non above the maximum": dict(n_non=MAX_SIDE + 1),
    }
    for what, change in bad.items():
        a = dict(good, **change)
        status = L.sat_eer_bootstrap_i32(a["ct"], a["cn"], a["K"], a["n_tar"], a["n_non"], a["first"], a["m"], 0, a["miss"], a["fa"], _lib.stream())
        assert status == -1, (what, status)                                       # SAT_ERR_INVALID
        assert b"eer_bootstrap" in L.sat_last_error(), (what, L.sat_last_error())
    torch.cuda.synchronize()
    assert bool((miss == -7).all()) and bool((fa == -9).all())                    # nothing ran
    a = good
    _lib.check(L.sat_eer_bootstrap_i32(a["ct"], a["cn"], a["K"], a["n_tar"], a["n_non"], 2 ** 31 - 1 - m, a["m"], 0, a["miss"], a["fa"], _lib.stream()), ENTRY)
    torch.cuda.synchronize()
    wm, wf = want(n_tar, n_non, "overlap", m, 0, 2 ** 31 - 1 - m)                 # the largest first_replicate the entry takes
    assert torch.equal(miss.cpu(), wm) and torch.equal(fa.cpu(), wf)


# ---- bounds: red zones around the four buffers of the call (tests/moat.py), as tests/test_hip_bounds.py does it ---------------------
@dataclass
class Row:
    entry: str                   # the C-ABI function
    name: str
    shapes: list
    make: object                 # make(*shape) -> (specs, call, ref)  (runs on the GPU box only)


ROWS = []


def _bounds_case(n_tar, n_non, kind, m):
    _lib = _sat()[0]
    ct, cn = cuts(n_tar, n_non, kind)
    K = len(ct) - 1
    specs = [Buf("cut_tar", "in", (K + 1,), I32, data=torch.from_numpy(ct)), Buf("cut_non", "in", (K + 1,), I32, data=torch.from_numpy(cn)),
             Buf("miss_at", "out", (m,), I32), Buf("fa_before", "out", (m,), I32)]

    def call(t):
        _lib.check(_lib.lib().sat_eer_bootstrap_i32(t["cut_tar"].data_ptr(), t["cut_non"].data_ptr(), K, n_tar, n_non, 0, m, 0, t["miss_at"].data_ptr(),
                                                    t["fa_before"].data_ptr(), _lib.stream()), ENTRY)
        assert _lib.lib().sat_last_dispatch_name().decode().split("<")[0].strip() == FAMILIES[0]

    def ref(t):
        wm, wf = want(n_tar, n_non, kind, m)
        assert torch.equal(t["miss_at"].cpu(), wm) and torch.equal(t["fa_before"].cpu(), wf)
    return specs, call, ref


ROWS.append(Row(ENTRY, "replicates", [c for c in TABLE if c[0] + c[1] <= 2 * 4097 and c[2] in ("overlap", "ties3")], _bounds_case))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [(r, s) for r in ROWS for s in r.shapes], ids=lambda p: f"{p[0].entry[4:]}:{p[0].name}-" + _id(p[1]))
def test_no_access_outside_the_buffers(p):
    r, shape = p
    specs, call, ref = r.make(*shape)
    v, m, plain = run_case(specs, call, DEV, sync=torch.cuda.synchronize)
    assert not v, f"{r.entry} [{r.name}] {shape}:\n" + "\n".join(str(x) for x in v)
    ref(m.t)


# ---- the command line on the toy data directory of tests/test_hip_asv_score.py ------------------------------------------------------
@pytest.mark.gpu
def test_asv_eval_command_line_writes_the_interval_and_prints_the_report(tmp_path, capsys):
    import json
    from satools_amd import asv_eval, pipeline, synthetic
    wavs = tmp_path / "wav"
    wavs.mkdir()
    enroll = {"spkA-u1": 0, "spkA-u2": 1, "spkB-u1": 2, "spkC-u1": 3, "spkC-u2": 4, "spkC-u3": 5}
    trial = {"spkA-u2": 1, "spkA-t1": 6, "spkB-t1": 7, "spkC-t1": 8, "spkB-t2": 9}
    for name, seed in {**enroll, **trial}.items():
        pipeline.save_pcm16(wavs / (name + ".wav"), synthetic.harm_utterance(seed, 16000 + 1601 * seed).unsqueeze(0), 16000)
    (tmp_path / "enroll.scp").write_text("".join(f"{n} {wavs / (n + '.wav')}\n" for n in enroll))
    (tmp_path / "trials.scp").write_text("".join(f"{n} {wavs / (n + '.wav')}\n" for n in trial))
    (tmp_path / "utt2spk").write_text("".join(f"{n} {n.split('-')[0]}\n" for n in enroll))
    (tmp_path / "trials").write_text("".join(f"{s} {u} {'target' if u.startswith(s) else 'nontarget'}\n" for s in ("spkA", "spkB", "spkC") for u in trial))
    args = ["synthetic:xvector?speakers=12", "--enrolls-wav-scp", str(tmp_path / "enroll.scp"), "--trails-wav-scp", str(tmp_path / "trials.scp"),
            "--enroll-utt2spk", str(tmp_path / "utt2spk"), "--trials", str(tmp_path / "trials")]
    asv_eval.main(args + ["--decode-output", str(tmp_path / "plain")])
    capsys.readouterr()
    asv_eval.main(args + ["--decode-output", str(tmp_path / "ci"), "--eer-ci", "10000", "--eer-ci-seed", "3", "--report"])
    printed = capsys.readouterr().out.splitlines()
    plain = json.load(open(tmp_path / "plain" / "metric.json"))
    ci = json.load(open(tmp_path / "ci" / "metric.json"))
    assert open(tmp_path / "plain" / "scores").read() == open(tmp_path / "ci" / "scores").read()
    try:
        import feerci  # noqa: F401
        return
    except ImportError:
        pass
    assert plain["eer_lower"] is None and plain["eer_upper"] is None and plain["asnorm"]["eer_lower"] is None          # without the option: as before
    for got, was in ((ci, plain), (ci["asnorm"], plain["asnorm"])):
        assert isinstance(got["eer_lower"], float) and isinstance(got["eer_upper"], float) and 0.0 <= got["eer_lower"] <= got["eer_upper"] <= 100.0
        assert got["eer"] >= was["eer"] - 1e-9                                    # the empirical EER, never below the ROCCH-EER
        assert all(got[k] == was[k] for k in ("linkability", "min_cllr", "eer_threshold"))
    assert set(ci) == set(plain) and set(ci["asnorm"]) == set(plain["asnorm"])
    assert printed[-2:] == asv_eval.report_lines(ci) and all(" ± " in l and l.startswith(" %EER: ") for l in printed[-2:])
