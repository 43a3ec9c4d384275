"""YAAPT beyond 2048 frames on the HIP device: sat_yaapt_long_f32 (csrc/yaapt_long/, include/satools_hip_yaapt_long.h), f0.yaapt_long, the
dispatch f0.track and the model calls behind it.  Needs a real MI355X: run with `-m gpu`.

1  THE LONG FORM IS THE RESIDENT FORM.  On every case of tests/yaapt_cases.py the entry point accepts (the raising ones and every option set
   included) the long form at chunk 64, 128 and the default has the bits of sat_yaapt_f32: every workspace view, the track, the status
   word, compared as int32 so that NaNs count.  With chunk 64 the catalogue's frame counts and candidate counts sit at chunk - 1, chunk,
   chunk + 1 and 2 chunk +- 1; `straddle64` puts a median window and a run of unvoiced frames across a chunk edge.
2  RAGGED: the 7- and 33-row batches of tests/test_hip_yaapt_stages.py equal sat_yaapt_ragged_f32 bit for bit.
3  BEYOND 2048 FRAMES (tests/yaapt_long_cases.py): the track equals the reference's (tests/golden/fx_f0_long.npz) on every frame but
   frame 0; spec_pitch / pitch_std equal oracle.spec_select of the device's candidates; the refined rows and the track equal oracle.refine +
   dynamic of the device's tp, tm, spec_pitch, energy, vuv (up to 4097 frames); the frame means hold the float64 bound of
   ref64_yaapt.judge_fmean; default chunk and chunk 512 agree bit for bit; the raising case gives status 1 and the reference's exception.
4  RAGGED BEYOND 2048: rows of 2049, 4097 and 65 frames and a NaN row equal their single calls, zero past each row's frames.
5  RED ZONES (tests/moat.py) around every buffer of sat_yaapt_long_f32: 2049 and 130 frames at chunk 64, plain and ragged.
6  REFUSALS with nothing launched and no sticky error.
7  END TO END: get_f0 / convert of both tags on the reference's 2049-frame fixture (tests/golden/fx_convert_long.npz), and the batch job on
   a 41 s file beside a 3 s file."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest
import torch

import moat
import yaapt_cases as yc
import yaapt_long_cases as ylc
from conftest import rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPTS = yc.OPTS
FBANK_TAG = "hifigan_bn_tdnnf_600h_vq_48_v1"
W2V2_TAG = "hifigan_bn_tdnnf_wav2vec2_vq_48_v1"
CHUNKS = (64, 128, 0)
_RESIDENT, _LONG = {}, {}


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---- the two entry points through the C ABI, each on a workspace of its own --------------------------------------------------------------
def entry(wav, opts, lengths=None, long=False, chunk=0):
    """-> (f0 [B, nf], status [B], {view: tensor}) on the CPU, of sat_yaapt_f32 / sat_yaapt_ragged_f32 (long=False) or sat_yaapt_long_f32"""
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    lib = _lib.lib()
    wav = wav.to(DEV, torch.float32).contiguous()
    B, n = wav.shape
    P = f0_hip.make_plan(n, dict(opts))
    hann, kaiser, tw = f0_hip._get_tables(P, wav.device)
    nws = lib.sat_yaapt_long_workspace_bytes(C.byref(P), B, chunk) if long else lib.sat_yaapt_workspace_bytes(C.byref(P), B)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=DEV)
    f0 = torch.empty(B, P.nframes, dtype=torch.float32, device=DEV)
    status = torch.empty(B, dtype=torch.int32, device=DEV)
    ud = None
    if lengths is not None:
        ud = torch.tensor([f0_hip.length_dims(P, int(v)) for v in lengths], dtype=torch.int32).to(DEV)
    p = _lib.ptr
    if long:
        rc = lib.sat_yaapt_long_f32(C.byref(P), p(wav), p(ud), p(f0), p(status), p(hann), p(kaiser), p(tw), p(ws), nws, B, chunk, _lib.stream())
    elif ud is None:
        rc = lib.sat_yaapt_f32(C.byref(P), p(wav), p(f0), p(status), p(hann), p(kaiser), p(tw), p(ws), nws, B, _lib.stream())
    else:
        rc = lib.sat_yaapt_ragged_f32(C.byref(P), p(wav), p(ud), p(f0), p(status), p(hann), p(kaiser), p(tw), p(ws), nws, B, _lib.stream())
    _lib.check(rc, "entry")
    torch.cuda.synchronize()
    return f0.cpu(), status.cpu(), {k: v.cpu() for k, v in f0_hip.workspace_views(ws, P, B).items()}


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same_run(a, b, what, rows=None):
    """track, status and every workspace view, as int32 bits.  `rows`: per row the frames it has (a ragged batch: the per-frame views of a
    shorter row are unwritten past its frames in BOTH forms; the track is zero there)"""
    (fa, sa, va), (fb, sb, vb) = a, b
    assert torch.equal(sa, sb), (what, "status", sa.tolist(), sb.tolist())
    assert torch.equal(bits(fa), bits(fb)), (what, "f0", torch.nonzero(bits(fa) != bits(fb))[:8].tolist())
    assert set(va) == set(vb)
    for k in va:
        x, y = bits(va[k]), bits(vb[k])
        if rows is not None and k not in ("filt", "scal"):
            for r, nf in enumerate(rows):
                assert torch.equal(x[r, ..., :nf], y[r, ..., :nf]), (what, k, r)
        elif rows is not None and k == "scal":
            assert torch.equal(x[:, :2], y[:, :2]), (what, k)
        else:
            if k == "scal":                  # pitch_std and the first failing NCCF frame; words 2 and 3 are never written
                x, y = x[:, :2], y[:, :2]
            assert torch.equal(x, y), (what, k, torch.nonzero(x != y)[:8].tolist())


# ---- 1: the long form is the resident form ---------------------------------------------------------------------------------------------
def _short_cases():
    cases = [c for c in yc.CASES if not c.refused] + [ylc.STRADDLE]
    cases += [c for s in yc.OPTION_SETS if not s.refused for c in s.cases]
    return cases


@pytest.mark.parametrize("case", _short_cases(), ids=repr)
def test_the_long_form_has_the_resident_forms_bits(case):
    wav = case.wav().unsqueeze(0)
    want = entry(wav, case.opts)
    assert want[0].shape == (1, case.nframes)
    if case.raises == "RuntimeError" and case.opts is OPTS:
        assert want[1].tolist() == [1]
    for chunk in CHUNKS:
        assert_same_run(entry(wav, case.opts, long=True, chunk=chunk), want, (case, chunk))


def test_the_straddle_case_straddles():
    """its unvoiced run lies across frame 64 and its compacted axis is shorter than its frame axis: the properties it is there for"""
    _, _, v = entry(ylc.STRADDLE.wav().unsqueeze(0), OPTS)
    has = v["cand"][0, 0] > 0
    gap = torch.nonzero(~has[1:-1]).flatten() + 1
    print("frames without a candidate:", gap.tolist())
    assert gap.numel() >= 3 and int(gap.min()) < 64 <= int(gap.max()) and 64 < int(has.sum()) < 130


# ---- 2: ragged ---------------------------------------------------------------------------------------------------------------------------
RAGGED_MIX = ["tone_1280", "tone_20160", "tone_20480", "tone_20481", "tone_41280", "burst260_at20220_of20480",
              "burst270_at8000_of20480"]        # tests/test_hip_yaapt_stages.py: 4, 63, 64, 65 and 129 frames, nv == 1 (NaN), nv == 2


@pytest.mark.parametrize("B", [len(RAGGED_MIX), 33])
def test_ragged_batches_have_the_bits_of_the_resident_ragged_form(B):
    cases = [yc.by_name(RAGGED_MIX[i % len(RAGGED_MIX)]) for i in range(B)]
    n_max = max(c.n for c in cases) + (1 if B == 33 else 0)
    wav = torch.zeros(B, n_max)
    for i, c in enumerate(cases):
        wav[i, :c.n] = c.wav()
    lens = [c.n for c in cases]
    want = entry(wav, OPTS, lengths=lens)
    for i, c in enumerate(cases):
        assert not want[0][i, c.nframes:].any()
    for chunk in CHUNKS:
        assert_same_run(entry(wav, OPTS, lengths=lens, long=True, chunk=chunk), want, (B, chunk), rows=[c.nframes for c in cases])


# ---- 3: beyond 2048 frames -----------------------------------------------------------------------------------------------------------------
def long_run(case, chunk=0):
    from satools_amd import f0 as f0_hip
    key = (case.name, chunk)
    if key not in _LONG:
        f0, aux = f0_hip.yaapt_long(case.wav().unsqueeze(0).to(DEV), case.opts, chunk_frames=chunk, return_aux=True)
        _LONG[key] = (f0.cpu()[0], {k: v.cpu()[0] for k, v in aux.items()})
    return _LONG[key]


def same(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("case", ylc.accepted(), ids=repr)
def test_beyond_2048_frames_against_the_reference_and_the_oracle(case, gold):
    from oracle import yaapt as oy
    fx = gold.npz("fx_f0_long.npz")
    assert case.nframes > ylc.MAX_RESIDENT and str(fx["raised/" + case.name]) == ""
    f0, g = long_run(case)
    f512, g512 = long_run(case, 512)
    assert torch.equal(bits(f0), bits(f512)), "default chunk against chunk 512"
    for k in g:
        x, y = bits(g[k]), bits(g512[k])
        assert torch.equal(x[:2] if k == "scal" else x, y[:2] if k == "scal" else y), ("default chunk against chunk 512", k)
    ref_track = torch.from_numpy(fx[case.name][0])
    diff = torch.nonzero(f0[1:] != ref_track[1:]).flatten() + 1
    print(f"\n{case.name}: {case.nframes} frames, {int((g['cand'][0] > 0).sum())} with a spectral candidate, frame 0 "
          f"{'equal' if f0[0] == ref_track[0] else 'differs'}; frames off the reference's track: {diff[:8].tolist()}")
    assert f0.shape == ref_track.shape == (case.nframes,) and diff.numel() == 0
    if case.name in ylc.FIXTURE_ONLY:
        return
    plan = oy.Plan(case.n, case.opts)
    nf = plan.nframes
    energy, vuv = g["energy"], g["vuv"].bool()
    cp, cm = g["cand"][:4], g["cand"][4:]
    spec, pstd = g["spec_pitch"], g["scal"][0]
    want_spec, want_std = oy.spec_select(cp.clone(), cm.clone(), plan)
    assert same(spec, want_spec), ("spec_pitch", torch.nonzero(spec != want_spec).flatten()[:8].tolist())
    assert same(pstd, want_std), ("pitch_std", float(pstd), float(want_std))
    z = torch.zeros(2, nf)
    tp1, tm1 = torch.cat((g["tp"][0:1], z)), torch.cat((g["tm"][0:1], z))
    tp2, tm2 = torch.cat((g["tp"][1:2], z)), torch.cat((g["tm"][1:2], z))
    rp, rm = oy.refine(tp1, tm1, tp2, tm2, spec.clone(), energy, vuv, plan)
    assert same(g["refined"][:6], rp), "refined pitch"
    assert same(g["refined"][6:], rm), "refined merit"
    want_f0 = oy.dynamic(rp, rm, energy, plan)
    assert same(f0, want_f0), ("final f0", torch.nonzero(f0 != want_f0).flatten()[:8].tolist())
    got = yc.check_properties(case, dict(energy=energy, vuv=vuv, cand_pitch=cp, pitch_std=pstd, ref_pitch=rp))
    print(f"{case.name}: {got}")


def test_frame_means_of_2049_frames_hold_the_float64_bound():
    import ref64_yaapt as r64
    from oracle import yaapt as oy
    from test_hip_yaapt_stages import DEVICE          # the rounding counts of the frame-mean kernel: the long form sums in the same order
    case = ylc.by_name("noisy1_655361")
    _, g = long_run(case)
    plan = oy.Plan(case.n, case.opts)
    for sig in (0, 1):
        res = r64.judge_fmean(g["filt"][sig].numpy(), g["fmean"][sig].numpy(), plan, DEVICE)
        print(f"fmean{sig + 1} of {case.name}: error / bound {res['ratio']:.4f}")
        assert not res.get("wrong") and res["ratio"] <= 1.0, (sig, res["ratio"])


@pytest.mark.parametrize("case", ylc.raising(), ids=repr)
def test_raises_where_the_reference_does_beyond_2048_frames(case, gold):
    from satools_amd import f0 as f0_hip
    assert str(gold.npz("fx_f0_long.npz")["raised/" + case.name]) == case.raises == "RuntimeError"
    for chunk in (0, 512):
        f0, st = f0_hip.yaapt_long(case.wav().unsqueeze(0).to(DEV), OPTS, chunk_frames=chunk, defer_status=True)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="no voiced frame"):
            st.check()
        assert st.words.tolist() == [1]
    with pytest.raises(RuntimeError, match="no voiced frame"):
        f0_hip.yaapt_long(case.wav().unsqueeze(0).to(DEV), OPTS)


# ---- 4: ragged beyond 2048 -----------------------------------------------------------------------------------------------------------------
def test_ragged_batch_beyond_2048_frames_rows_are_their_single_tracks():
    from satools_amd import f0 as f0_hip
    cases = [ylc.by_name("tone_655361"), ylc.by_name("gated2_1310721"), yc.by_name("tone_20481"), yc.by_name("burst260_at20220_of20480")]
    n_max = max(c.n for c in cases)
    wav = torch.zeros(len(cases), n_max)
    for i, c in enumerate(cases):
        wav[i, :c.n] = c.wav()
    got = f0_hip.yaapt_long(wav.to(DEV), OPTS, lengths=[c.n for c in cases]).cpu()
    also = f0_hip.track(wav.to(DEV), OPTS, lengths=[c.n for c in cases]).cpu()         # the dispatch: the long form for every row
    assert got.shape == (len(cases), math.ceil(n_max / 320)) and torch.equal(bits(got), bits(also))
    _, _, v = entry(cases[3].wav().unsqueeze(0), OPTS)
    assert bool(torch.isnan(v["tm"]).all())                                           # the NaN row: every NCCF merit of it is NaN
    for i, c in enumerate(cases):
        one = long_run(c)[0] if c.nframes > ylc.MAX_RESIDENT else entry(c.wav().unsqueeze(0), OPTS)[0][0]
        assert torch.equal(bits(got[i, :c.nframes]), bits(one)), (i, c, torch.nonzero(got[i, :c.nframes] != one).flatten()[:8].tolist())
        assert not got[i, c.nframes:].any(), (i, c)


# ---- 5: red zones --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ragged", [(655361, False), (655361, True), (41281, False), (41281, True)], ids=str)
def test_red_zones_around_every_buffer_of_the_long_entry_point(n, ragged):
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    lib = _lib.lib()
    B, chunk = (2 if ragged else 1), 64
    P = f0_hip.make_plan(n, dict(OPTS))
    wav = torch.stack([yc.noisy_tone(3 + b, n) for b in range(B)])
    lens = [n, n - 20000][:B]
    if ragged:
        wav[1, lens[1]:] = 0.0
    nws = lib.sat_yaapt_long_workspace_bytes(C.byref(P), B, chunk)
    hann = torch.hann_window(P.frame_size + 2)[1:-1].contiguous()
    kaiser = torch.kaiser_window(P.nframe_size, periodic=True, beta=0.5)
    k = np.arange(4096, dtype=np.float64)
    tw = torch.from_numpy(np.stack([np.cos(2 * np.pi * k / 8192.0), -np.sin(2 * np.pi * k / 8192.0)], 1).astype(np.float32))
    dims = torch.tensor([f0_hip.length_dims(P, v) for v in lens], dtype=torch.int32)
    specs = [moat.Buf("wav", "in", (B, n), data=wav), moat.Buf("f0", "out", (B, P.nframes)),
             moat.Buf("status", "out", (B,), dtype=torch.int32), moat.Buf("hann", "in", tuple(hann.shape), data=hann),
             moat.Buf("kaiser", "in", tuple(kaiser.shape), data=kaiser), moat.Buf("twiddle", "in", (4096, 2), data=tw),
             moat.Buf("workspace", "workspace", (nws,), dtype=torch.uint8)]
    if ragged:
        specs.append(moat.Buf("utt_dims", "in", (B, 4), dtype=torch.int32, data=dims))
    p = _lib.ptr

    def call(t):
        _lib.check(lib.sat_yaapt_long_f32(C.byref(P), p(t["wav"]), p(t["utt_dims"]) if ragged else None, p(t["f0"]), p(t["status"]), p(t["hann"]),
                                          p(t["kaiser"]), p(t["twiddle"]), p(t["workspace"]), nws, B, chunk, _lib.stream()), "sat_yaapt_long_f32")

    v, m, plain = moat.run_case(specs, call, device=DEV, sync=torch.cuda.synchronize)
    assert not v, [str(x) for x in v]
    assert m.t["status"].tolist() == [0] * B and bool((plain["f0"] > 0).any())
    if ragged:
        assert not m.t["f0"][1, dims[1, 2]:].any()


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(n, match, chunk=0, shortfall=None, code=None):
    """sat_yaapt_long_f32 on sentinel-filled outputs: refused with `match`, and neither output was touched"""
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    lib = _lib.lib()
    P = f0_hip.make_plan(n, dict(OPTS))
    hann, kaiser, tw = f0_hip._get_tables(P, torch.device(DEV))
    wav = torch.zeros(1, n, device=DEV)
    nws = lib.sat_yaapt_long_workspace_bytes(C.byref(P), 1, chunk) if shortfall is not None else 4096
    ws = torch.empty(max(nws, 4096), dtype=torch.uint8, device=DEV)
    f0 = torch.full((1, P.nframes), -7.0, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    rc = lib.sat_yaapt_long_f32(C.byref(P), p(wav), None, p(f0), p(status), p(hann), p(kaiser), p(tw), p(ws), nws - (shortfall or 0), 1, chunk, _lib.stream())
    with pytest.raises(_lib.SatError, match=match):
        _lib.check(rc, "sat_yaapt_long_f32")
    assert rc == (code if code is not None else -1)
    torch.cuda.synchronize()
    assert bool((f0 == -7.0).all()) and status.tolist() == [-7]
    return P


def test_refusals_launch_nothing_and_leave_no_sticky_error():
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    lib = _lib.lib()
    invalid, workspace = -1, -3                                     # SAT_ERR_INVALID, SAT_ERR_WORKSPACE (include/satools_hip.h)
    assert _refused(960, r"yaapt_long: 3 frames not supported \(4 frames at least\)", code=invalid).nframes == 3
    n_cap = 26211 * 320                                            # 64 * Lz * 4 < 2^31 with Lz = 1120 + (frames - 1) * 320
    assert f0_hip.long_frames_ok(f0_hip.make_plan(n_cap, dict(OPTS))) and f0_hip.make_plan(n_cap, dict(OPTS)).nframes == 26211
    P = _refused(n_cap + 1, r"yaapt_long: 26212 frames not supported: utterance too long for the prefilter's 31-bit row offsets", code=invalid)
    assert not f0_hip.long_frames_ok(P)
    _refused(655361, r"yaapt_long: chunk_frames 96 not supported", chunk=96, code=invalid)
    for chunk in (32, 2112, -64):
        assert lib.sat_yaapt_long_workspace_bytes(C.byref(P), 1, chunk) == 0
    _refused(655361, "yaapt_long: workspace too small", shortfall=1, code=workspace)
    with pytest.raises(_lib.SatError, match=r"chunk_frames 96 not supported"):
        f0_hip.yaapt_long(torch.zeros(1, 655361, device=DEV), OPTS, chunk_frames=96)
    with pytest.raises(_lib.SatError, match=r"26212 frames not supported"):
        f0_hip.yaapt_long(torch.zeros(1, n_cap + 1, device=DEV), OPTS)
    case = ylc.by_name("tone_655361")
    with pytest.raises(_lib.SatError, match=r"yaapt: 2049 frames not supported \(4\.\.2048, i\.e\. up to ~40 s\)"):
        f0_hip.yaapt(case.wav().unsqueeze(0).to(DEV), OPTS)
    small = yc.by_name("tone_1280")
    again = f0_hip.yaapt_long(small.wav().unsqueeze(0).to(DEV), OPTS).cpu()
    torch.cuda.synchronize()
    assert torch.equal(bits(again), bits(entry(small.wav().unsqueeze(0), OPTS)[0]))


# ---- 7: end to end ---------------------------------------------------------------------------------------------------------------------------
def _long_batch(seeds, n):
    """tests/test_hip_robust.py: `harm` utterances longer than the generator's 5 s period, seeds change every 5 s segment"""
    from satools_amd import synthetic
    rows = []
    for s in seeds:
        segs = [synthetic.harm_batch([s + 7 * j], 80000)[0] for j in range((n + 79999) // 80000)]
        rows.append(torch.cat(segs)[:n])
    return torch.stack(rows)


def _model(tag):
    import satools_amd
    m = satools_amd.load_model("synthetic:" + tag)
    m.to(DEV)
    m.eval()
    return m


def _fixture_wav(fx):
    from satools_amd import synthetic
    n = int(fx["n"])
    wav = torch.cat([synthetic.harm_batch([int(sd)], 80000)[0] for sd in fx["seeds"]])[:n].unsqueeze(0)
    assert torch.equal(wav, _long_batch([int(fx["seeds"][0])], n)) and n == 655361
    return n, wav


def test_convert_41s_fbank_tag_against_the_reference_fixture(gold):
    fx = gold.npz("fx_convert_long.npz")
    n, wav = _fixture_wav(fx)
    model = _model(FBANK_TAG)
    f0 = model.get_f0(wav.to(DEV)).cpu()
    assert f0.shape == (1, 2049) and np.array_equal(f0.numpy()[:, 1:], fx["fbank/f0"][:, 1:])
    # the index rule of test_convert_20s_wav2vec2_tag_against_the_reference_fixture (see the next test)
    ext = model.bn_extractor
    ref_idx = torch.from_numpy(fx["fbank/idx"]).long().flatten()
    d1, d2 = torch.from_numpy(fx["fbank/d1"]).double().flatten().clamp_min(0), torch.from_numpy(fx["fbank/d2"]).double().flatten().clamp_min(0)
    _, (z, idx, _) = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
    with ext._exact(ext):
        _, (z32, idx32, _) = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
    rows = lambda t: t.permute(0, 2, 1).reshape(-1, t.shape[1]).cpu().double()
    flips32 = torch.nonzero(idx32.cpu().long().flatten() != ref_idx).flatten()
    flips = torch.nonzero(idx.cpu().long().flatten() != ref_idx).flatten()
    dz = (rows(z) - rows(z32)).norm(dim=1)
    bound = 2 * dz * (d1.sqrt() + d2.sqrt()) + 2 * dz ** 2
    print(f"41 s fbank fixture: {ref_idx.numel()} frames; index flips vs the reference: exact-f32 kernels {flips32.tolist()}, as configured "
          f"{flips.tolist()} (reference gaps {(d2 - d1)[flips].tolist()}, allowed {bound[flips].tolist()})")
    assert flips32.numel() == 0
    assert flips.numel() <= 2 and ((d2 - d1)[flips] <= bound[flips]).all()
    y = model.convert(wav.to(DEV), target=model.spk[5])
    assert y.shape == (1, 2048 * 320 + 1)                         # 2048 bottleneck frames (the F0 track's 2049th is cropped), 320 samples each
    ref_y = torch.from_numpy(fx["fbank/convert_every16"]).reshape(-1)
    got_y = y.cpu().reshape(-1)[::16]
    assert got_y.shape == ref_y.shape
    keep = torch.ones(got_y.shape[-1], dtype=torch.bool)
    for f in flips.tolist():                                    # (a flipped code changes ~40 frames of output around it)
        keep[max(0, (f - 40) * 20):(f + 40) * 20] = False
    err = rms((got_y - ref_y)[keep].numpy())
    print(f"41 s fbank fixture: waveform RMS error vs the reference {err:.2e} on {int(keep.sum())} of {keep.numel()} stored samples")
    assert err < 1e-5


def test_convert_41s_wav2vec2_tag_against_the_reference_fixture(gold):
    """the rule of tests/test_hip_robust.py::test_convert_20s_wav2vec2_tag_against_the_reference_fixture: the exact-f32 kernels reproduce
    every index; the split-f16 kernels may differ only where the reference's two best distances are closer than the kernel's own
    measured error (its distance to its exact-f32 twin)"""
    fx = gold.npz("fx_convert_long.npz")
    n, wav = _fixture_wav(fx)
    model = _model(W2V2_TAG)
    ext = model.bn_extractor
    ref_idx = torch.from_numpy(fx["w2v2/idx"]).long().flatten()
    d1, d2 = torch.from_numpy(fx["w2v2/d1"]).double().flatten().clamp_min(0), torch.from_numpy(fx["w2v2/d2"]).double().flatten().clamp_min(0)
    zs, flips = {}, {}
    for mode in ("f32", "f16x3"):
        keep_cfg = {k: getattr(ext, k) for k in ("precision", "w2v2_precision")}
        try:
            if mode == "f32":
                ext.precision = ext.w2v2_precision = "f32"
            _, (z, idx, _) = ext.extract_bn(wav.clone().to(DEV), want_aux=True)
        finally:
            for k, v in keep_cfg.items():
                setattr(ext, k, v)
        zs[mode] = z.permute(0, 2, 1).reshape(-1, z.shape[1]).cpu().double()
        flips[mode] = torch.nonzero(idx.cpu().long().flatten() != ref_idx).flatten()
    dz = (zs["f16x3"] - zs["f32"]).norm(dim=1)
    bound = 2 * dz * (d1.sqrt() + d2.sqrt()) + 2 * dz ** 2
    print(f"41 s wav2vec2 fixture: {ref_idx.numel()} frames; index flips vs the reference: exact-f32 kernels {flips['f32'].tolist()}, split-f16 kernels "
          f"{flips['f16x3'].tolist()} (reference gaps {[f'{g:.1e}' for g in (d2 - d1)[flips['f16x3']].tolist()]}, allowed by the measured error "
          f"{[f'{g:.1e}' for g in bound[flips['f16x3']].tolist()]})")
    assert flips["f32"].numel() == 0
    assert flips["f16x3"].numel() <= 2 and ((d2 - d1)[flips["f16x3"]] <= bound[flips["f16x3"]]).all()
    f0 = model.get_f0(wav.to(DEV)).cpu()
    assert f0.shape == (1, 2049) and np.array_equal(f0.numpy()[:, 1:], fx["w2v2/f0"][:, 1:])
    y = model.convert(wav.to(DEV), target=model.spk[5])
    assert y.shape == (1, 2048 * 320 + 1)                         # 2048 bottleneck frames (the F0 track's 2049th is cropped), 320 samples each
    ref_y = torch.from_numpy(fx["w2v2/convert_every16"]).reshape(-1)
    got_y = y.cpu().reshape(-1)[::16]
    assert got_y.shape == ref_y.shape
    keep = torch.ones(got_y.shape[-1], dtype=torch.bool)
    for f in flips["f16x3"].tolist():                           # (a flipped code changes ~40 frames of output around it)
        keep[max(0, (f - 40) * 20):(f + 40) * 20] = False
    err = rms((got_y - ref_y)[keep].numpy())
    print(f"41 s wav2vec2 fixture: waveform RMS error vs the reference {err:.2e} on {int(keep.sum())} of {keep.numel()} stored samples")
    assert err < 1e-4


def test_a_41_s_file_beside_a_3_s_file_through_process_data(tmp_path):
    """the batch job on a wav.scp with one file beyond 2048 frames: every file holds the PCM16 bits of convert_padded() of the same batch"""
    from pipeline_toy import read_wav, write_wav
    from satools_amd import pipeline as pl
    model = _model(FBANK_TAG)
    data = str(tmp_path / "data" / "long")
    os.makedirs(os.path.join(data, "clear"), exist_ok=True)
    lens = [41 * 16000, 3 * 16000]
    scp, u2s = [], []
    for i, n in enumerate(lens):
        path = os.path.join(data, "clear", f"utt{i}.wav")
        write_wav(path, _long_batch([20 + i], n)[0].numpy().astype(np.float64))
        scp.append(f"utt{i} {path}\n")
        u2s.append(f"utt{i} src{i}\n")
    open(os.path.join(data, "wav.scp"), "w").writelines(scp)
    open(os.path.join(data, "utt2spk"), "w").writelines(u2s)
    target = model.spk[11]
    settings = types.SimpleNamespace(model="-", f0_modification="", target_constant_spkid=target, results_dir="wav",
                                     batch_size=2, data_loader_nj=2, new_datadir_suffix="_anon", device="cuda")
    table = pl.read_wav_scp(os.path.join(data, "wav.scp"))
    assert pl.process_data(data, "constant", table, settings, model=model) == 2
    x = torch.zeros(2, max(lens))
    for i, n in enumerate(lens):
        x[i, :n] = pl.load_wav_from_scp(table[f"utt{i}"])[0][0]
    ref = model.convert_padded(x.to(DEV), lens, [target] * 2).cpu()
    one = model.convert(x[:1].to(DEV), target=target).cpu().reshape(-1)       # and the long row alone: the plain long call
    assert torch.isfinite(ref).all() and one.shape[0] == lens[0] + 1
    for i, n in enumerate(lens):
        got, sr = read_wav(os.path.join(data + "_anon", "wav", f"utt{i}.wav"))
        exp = np.clip(np.rint(ref[i, 0, :n].numpy().astype(np.float64) * 32768), -32768, 32767).astype(np.int16)
        assert sr == 16000 and got.shape == (n,) and np.array_equal(got, exp), i
