"""Host side of YAAPT beyond 2048 frames (csrc/yaapt_long/, include/satools_hip_yaapt_long.h), CPU only: the catalogue of
tests/yaapt_long_cases.py held against the float32 oracle and the reference's tracks (tests/golden/fx_f0_long.npz), the chunk walk of the
long kernels restated in plain Python with its constants pinned to the source, and the dispatch f0.track (header, binding and build are
held together by tests/test_components_host.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import yaapt_cases as yc
import yaapt_long_cases as ylc
from satools_amd import _lib
from satools_amd import f0 as f0_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sa-toolkit_amd", "csrc")
HEADER = "satools_hip_yaapt_long.h"
SOURCE = os.path.join(CSRC, "yaapt_long", "yaapt_long.hip")


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)          # the reference's own YAAPT setting; frame 0 depends on the thread count
    yield
    torch.set_num_threads(n)


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------------
def test_the_catalogue_has_the_cases_the_long_form_is_there_for():
    frames = {c.name: c.nframes for c in ylc.CASES}
    assert frames == {"tone_655361": 2049, "noisy1_655361": 2049, "gated2_660000": 2063, "jump_700000": 2188, "gated2_1310721": 4097,
                      "noisy1_2621441": 8193, "burst60_at8000_of655361": 2049, "burst270_at8000_of655361": 2049}
    assert all(n > ylc.MAX_RESIDENT == f0_hip.MAX_RESIDENT_FRAMES == yc.MAX_FRAMES for n in frames.values())
    assert [c.name for c in ylc.raising()] == ["burst60_at8000_of655361"] and ylc.FIXTURE_ONLY == ("noisy1_2621441",)
    assert max(c.nframes for c in ylc.oracle_checked()) == 4097
    assert torch.equal(ylc.by_name("tone_655361").wav(), yc.by_name("tone_655361").wav())
    g = ylc.gated(torch.ones(2 * 64000))
    assert g[:48000].all() and not g[48000:64000].any() and g[64000:112000].all() and not g[112000:].any()      # 3 s on, 1 s off
    for c in ylc.CASES + [ylc.STRADDLE]:
        assert f0_hip.plan_frames(c.n, c.opts) == c.nframes == f0_hip.make_plan(c.n, dict(c.opts)).nframes, c


@pytest.mark.parametrize("case", ylc.CASES, ids=repr)
def test_declared_properties_and_the_references_track_from_the_oracle(case, gold):
    """frame count, nv, the raising case — from oracle.yaapt.yaapt_one; and its track IS the reference's (every frame, one thread)"""
    fx = gold.npz("fx_f0_long.npz")
    aux, final, raised = yc.oracle_run(case)
    got = yc.check_properties(case, aux)
    print(f"\n{case.name}: {got} raised={raised!r}")
    assert raised == (case.raises or "") == str(fx["raised/" + case.name])
    if case.raises:
        assert got["nv"] == 0 and case.name not in fx
        return
    assert np.array_equal(final.numpy(), fx[case.name][0])
    if case.name == "gated2_660000":        # the compaction differs from the frame count: well under half of the frames carry a candidate
        assert 700 <= got["nv"] <= 1000, got
    if case.name == "burst270_at8000_of655361":
        assert got["nv"] in (1, 2) and got["mean_nan"]


def test_the_straddle_case_declares_130_frames():
    x = ylc.STRADDLE.wav()
    assert ylc.STRADDLE.nframes == 130 and not x[61 * 320 + 100:66 * 320 + 200].any() and x[:61 * 320].any() and x[67 * 320:].any()


# ---- what is particular to this component (tests/test_components_host.py holds header, binding, library and build together) ---------------
def test_f0_has_the_long_form_and_the_build_depends_on_the_headers_it_shares_with_the_resident_form():
    from satools_amd import build
    assert callable(f0_hip.yaapt_long) and callable(f0_hip.track)
    for shared in ("yaapt_dev.h", "yaapt_spec_select_body.h", "yaapt_refine_body.h"):
        assert any(h.endswith(os.sep + shared) for h in build.headers()), shared


def test_workspace_bytes_and_the_chunk_set_without_a_gpu():
    """the size function is host arithmetic: the resident layout, then ARENA_FLOATS floats per (utterance, frame); 0 outside the chunk set"""
    lib = _lib.lib()
    for n, B in ((655361, 1), (41281, 3)):
        P = f0_hip.make_plan(n, dict(yc.OPTS))
        head = lib.sat_yaapt_workspace_bytes(C.byref(P), B)
        for chunk in (0, 64, 512, 2048):
            got = lib.sat_yaapt_long_workspace_bytes(C.byref(P), B, chunk)
            # (both sizes are rounded up to 256 bytes, the head's before the arena is added here)
            assert got % 256 == 0 and -256 < got - (head + 4 * ylc.ARENA_FLOATS * B * P.nframes) < 256 and ylc.valid_chunk(chunk)
        for chunk in (-64, 1, 32, 96, 2049, 2112, 4096):
            assert lib.sat_yaapt_long_workspace_bytes(C.byref(P), B, chunk) == 0 and ylc.valid_chunk(chunk) is None
        assert lib.sat_yaapt_long_workspace_bytes(C.byref(P), 0, 0) == 0 and lib.sat_yaapt_long_workspace_bytes(None, 1, 0) == 0


# ---- the chunk walk ------------------------------------------------------------------------------------------------------------------------
def _src(path):
    return re.sub(r"\s+", " ", open(path).read())


def test_the_walks_constants_are_the_sources():
    text, header = _src(SOURCE), _src(os.path.join(ROOT, "include", HEADER))
    d = {k: int(v) for k, v in re.findall(r"#define SAT_YAAPT_LONG_(\w+) (\d+)", header)}
    assert d == {"DEFAULT_CHUNK": ylc.DEFAULT_CHUNK, "MAX_CHUNK": ylc.MAX_CHUNK, "SCRATCH_FLOATS": ylc.ARENA_FLOATS}
    assert (f0_hip.LONG_CHUNK_STEP, f0_hip.LONG_DEFAULT_CHUNK, f0_hip.LONG_MAX_CHUNK) == (ylc.CHUNK_STEP, ylc.DEFAULT_CHUNK, ylc.MAX_CHUNK)
    assert int(re.search(r"constexpr int YL_CHUNK_STEP = (\d+);", text).group(1)) == ylc.CHUNK_STEP == 64
    assert int(re.search(r"constexpr int YL_HALO = (\d+);", text).group(1)) == ylc.HALO == 1
    for name, macro in (("YL_CHUNK_DEFAULT", "SAT_YAAPT_LONG_DEFAULT_CHUNK"), ("YL_CHUNK_MAX", "SAT_YAAPT_LONG_MAX_CHUNK"), ("YL_ARENA", "SAT_YAAPT_LONG_SCRATCH_FLOATS")):
        assert re.search(r"constexpr int " + name + " = " + macro + ";", text), name
    dev = _src(os.path.join(CSRC, "yaapt_dev.h"))
    assert int(re.search(r"constexpr int YAAPT_MAX_RESIDENT_FRAMES = (\d+);", dev).group(1)) == ylc.MAX_RESIDENT
    assert "P.nframes <= YAAPT_MAX_RESIDENT_FRAMES" in _src(os.path.join(CSRC, "yaapt.hip"))
    # the walk itself: chunk starts, the staged range, the first recursion frame, the reverse walk
    assert "for (int c0 = 0; c0 < T; c0 += CH) { const int n = min(CH, T - c0);" in text
    assert "for (int q = lane; q < n + YL_HALO; q += 64) { const int t = c0 - YL_HALO + q; if (t >= 0) {" in text
    assert "for (int t = c0 > 1 ? c0 : 1; t < c0 + n; ++t) { const int q = t - c0 + YL_HALO;" in text
    assert "for (int c0 = ((T - 1) / CH) * CH; c0 >= 0; c0 -= CH) {" in text
    assert "for (int u = c0 + n - 1; u >= (c0 > 1 ? c0 : 1); --u) {" in text and "path_out[u - 1] = (unsigned char)p;" in text
    # the dynamic LDS the launcher asks for
    assert "const size_t SP = (size_t)CH + YL_HALO;" in text
    assert "const size_t post_lds = 2 * 4 * SP * sizeof(float) + 4 * (size_t)CH;" in text
    assert "const size_t dp_lds = (2 * NC + 1) * SP * sizeof(float) + NC * (size_t)CH;" in text
    assert ylc.lds_bytes(ylc.MAX_CHUNK)["refine_dp"] <= 160 * 1024 and "160 * 1024" in text
    # both forms include the same statements
    for body in ("yaapt_spec_select_body.h", "yaapt_refine_body.h"):
        assert f'#include "../{body}"' in text and f'#include "{body}"' in _src(os.path.join(CSRC, "yaapt.hip")), body
    # the arena holds what the bodies lay out: 53 and 63 bytes per frame
    assert 4 * ylc.ARENA_FLOATS >= max((4 + 4 + 3) * 4 + 2 * 2 + 5, (2 * 6 + 2) * 4 + 7)


@pytest.mark.parametrize("T,CH", [(3, 64), (63, 64), (64, 64), (65, 64), (127, 64), (128, 64), (129, 64), (130, 64), (2049, 64), (2049, 1024),
                                  (4097, 1024), (4097, 512), (8193, 2048)])
def test_the_walk_covers_every_frame_once_and_carries_across_the_edges(T, CH):
    w = ylc.walk(T, CH)
    assert [c["c0"] for c in w] == list(range(0, T, CH)) and sum(c["n"] for c in w) == T
    steps = [t for c in w for t in c["steps"]]
    assert steps == list(range(1, T))                                 # every frame but frame 0 takes one recursion step, in order
    for c in w:
        assert len(c["staged"]) <= CH + ylc.HALO
        for t in c["steps"]:
            assert t in c["staged"] and t - 1 in c["staged"]          # the step reads frames t and t - 1 from the staged chunk
        assert c["pred"] == c["steps"]
    back = ylc.walk_back(T, CH)
    assert [c["c0"] for c in back] == list(range(0, T, CH))[::-1]
    assert [t for c in back for t in c["path"]] == list(range(T - 2, -1, -1))       # path[T - 1] first, then every frame once, downwards
    for c in back:
        assert all(t + 1 in c["loaded"] for t in c["path"])           # path[t] = pred[p][t + 1], from the chunk that holds frame t + 1
    if len(back) > 1:
        assert back[0]["path"][-1] == back[0]["c0"] - 1               # the step out of a chunk's first frame writes the chunk before it
    means = ylc.walk_means(T, CH)
    assert [f for c in means for f in c["frames"]] == list(range(T)) and all(c["prefetched"] == c["frames"][-1] + 1 for c in means)


def test_lane_sums_do_not_depend_on_the_chunk():
    """the float64 sums are lane-strided by 64 from frame 0, and every chunk is a multiple of 64: lane l adds frames l, l + 64, ... in that
    order whatever the chunk is"""
    T = 2049
    for CH in (64, 512, 1024):
        assert CH % 64 == 0
        per_lane = {}
        for c0 in range(0, T, CH):
            for f in range(c0, min(c0 + CH, T)):
                per_lane.setdefault((f - c0) % 64, []).append(f)
        assert all(v == list(range(l, T, 64)) for l, v in per_lane.items())


# ---- the dispatch --------------------------------------------------------------------------------------------------------------------------
def test_track_routes_by_the_batch_plans_frames(monkeypatch):
    calls = []
    monkeypatch.setattr(f0_hip, "yaapt", lambda wav, opts, defer_status=False: calls.append(("yaapt", defer_status)))
    monkeypatch.setattr(f0_hip, "yaapt_ragged", lambda wav, lengths, opts, defer_status=False: calls.append(("ragged", defer_status)))
    monkeypatch.setattr(f0_hip, "yaapt_long", lambda wav, opts, lengths=None, defer_status=False: calls.append(("long", lengths, defer_status)))
    short, long = torch.zeros(2, 655360), torch.zeros(2, 655361)
    f0_hip.track(short, yc.OPTS)
    f0_hip.track(short, yc.OPTS, lengths=[100000, 655360], defer_status=True)
    f0_hip.track(long, yc.OPTS, defer_status=True)
    f0_hip.track(long, yc.OPTS, lengths=[3200, 655361])               # the longest row decides for every row
    assert calls == [("yaapt", False), ("ragged", True), ("long", None, True), ("long", [3200, 655361], False)]
    for n in (1280, 20481, 655360, 655361, 1310721):
        for opts in (yc.OPTS, {}, yc.option_set("sr22050").opts, yc.option_set("jump512_ov128").opts):
            assert f0_hip.plan_frames(n, opts) == f0_hip._derive_plan(n, dict(opts)).nframes, (n, opts)


def test_the_model_calls_go_through_track():
    text = open(os.path.join(ROOT, "sa-toolkit_amd", "anonymizer.py")).read()
    assert text.count("f0_hip.track(") == 4 and "f0_hip.yaapt(" not in text and "f0_hip.yaapt_ragged(" not in text


def test_long_frames_ok_is_the_prefilters_limit():
    P = f0_hip.make_plan(26211 * 320, dict(yc.OPTS))
    assert P.nframes == 26211 and f0_hip.long_frames_ok(P) and 64 * P.Lz * 4 < 2 ** 31
    P = f0_hip.make_plan(26211 * 320 + 1, dict(yc.OPTS))
    assert P.nframes == 26212 and not f0_hip.long_frames_ok(P) and 64 * P.Lz * 4 >= 2 ** 31
    assert "(size_t)64 * P.Lz * 4 < ((size_t)1 << 31)" in _src(SOURCE)
