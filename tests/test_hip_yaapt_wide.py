"""YAAPT on the HIP device at option sets whose time-domain frames overlap more than their predecessor (tests/yaapt_wide_cases.py: the
reference's defaults, three frames deep at a 10 ms hop; one and two frames deep; the cap of seven): the wide frame-means and NCCF kernels of
csrc/yaapt_long/yaapt_long.hip behind sat_yaapt_long_f32, f0.yaapt_long, the dispatch f0.track and the model calls.  Needs a real MI355X:
run with `-m gpu` (`-s` prints the error / bound ratios and the exempt frames).

1  STAGES.  Every accepted case runs ONCE through f0.yaapt_long(..., return_aux=True) and each stage is checked from the device's own
   upstream intermediates: `fmean` within the float64 bound of tests/ref64_yaapt_wide.py, frame by frame from the device's previous D means,
   with the rounding counts of the wide kernel (DEVICE_WIDE below, read off the source); `tp` / `tm` as ref64_yaapt.judge_nccf judges them,
   from frames rebuilt with the device's means; spec_pitch / pitch_std, the refined rows and the track equal to the oracle stages fed with
   the device's intermediates; the track equal to the reference's (tests/golden/fx_f0_wide.npz), frame 0 apart.
2  The raising case ends with the reference's exception through F0Status.
3  CHUNKS 64 and 128 against the default, bit for bit, every view of the workspace (65, 129 and 2049 frames among the cases).
4  RAGGED: rows of 65, 129, 2049 and 128 frames and a NaN row under the defaults equal their single calls, zero past each row's frames.
5  RED ZONES (tests/moat.py) around every buffer, `defaults` and `d7`, plain and ragged.
6  `d8` (eight frames deep) is refused by name with its outputs untouched; the next valid call is unchanged.
7  END TO END: get_f0 / convert of one tag whose f0_yaapt_opts are the reference's defaults."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import moat
import ref64_yaapt_wide as r64w
import yaapt_cases as yc
import yaapt_wide_cases as ywc
from test_hip_yaapt_long import FBANK_TAG, _model, assert_same_run, bits, entry, same
from test_hip_yaapt_stages import DEVICE          # the rounding counts of the kernels the wide form shares with the resident one (NCCF)

pytestmark = pytest.mark.gpu
DEV = "cuda"
_RUN, _RATIOS = {}, {}

# Rounding counts of yaapt_long_wide_frame_means_kernel, read off csrc/yaapt_long/yaapt_long.hip (ov = n - hop):
#   head  a lane adds the in-flight positions it owns, at most ceil(max(ov - hop, 0) / 64), then the raw ones, at most
#         ceil(min(hop, ov) / 64), into one accumulator; six shuffle levels.  (Frame 0's head: ceil(ov / 64) adds, not more than that.)
#         The subtractions a term has been through are counted one by one by the reference itself.
#   tail  ceil(hop / 64) adds per lane, six shuffle levels (yaapt_long_frame_means_kernel's)
_c = math.ceil
DEVICE_WIDE = r64w.WideRoundings(head=lambda n, hop: _c(max(n - 2 * hop, 0) / 64) + _c(min(hop, n - hop) / 64) + 6,
                                 tail=lambda n, hop: _c(hop / 64) + 6)


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def run(case, chunk=0):
    from satools_amd import f0 as f0_hip
    key = (case.name, chunk)
    if key not in _RUN:
        f0, aux = f0_hip.yaapt_long(case.wav().unsqueeze(0).to(DEV), case.opts, chunk_frames=chunk, return_aux=True)
        _RUN[key] = (f0.cpu()[0], {k: v.cpu()[0] for k, v in aux.items()})
    return _RUN[key]


# ---- 1: the stages -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ywc.accepted(), ids=repr)
def test_stages_from_the_devices_own_intermediates_and_the_references_track(case, gold):
    from oracle import yaapt as oy
    fx = gold.npz("fx_f0_wide.npz")
    assert str(fx["raised/" + case.name]) == ""
    f0, g = run(case)
    plan = oy.Plan(case.n, case.opts)
    nf = plan.nframes
    assert f0.shape == (nf,) == (case.nframes,) and plan.tda_nframes == nf
    filt = g["filt"].numpy()
    spec, pstd = g["spec_pitch"], g["scal"][0]
    for sig in (0, 1):
        fm = g["fmean"][sig].numpy()
        res = r64w.judge_fmean_wide(filt[sig], fm, plan, DEVICE_WIDE)
        nc = r64w.judge_nccf_wide(filt[sig], fm, spec.numpy(), float(pstd), g["tp"][sig].numpy(), g["tm"][sig].numpy(), plan, DEVICE)
        _RATIOS[(case.name, sig)] = (res["ratio"], nc["ratio"])
        print(f"\n{case.name} signal {sig + 1}: fmean error / bound {res['ratio']:.4f}; nccf error / bound {nc['ratio']:.4f}, exempt "
              f"{nc['exempt'][:12]}{' ..' if len(nc['exempt']) > 12 else ''} ({len(nc['exempt'])}), unbounded {nc['unbounded']}")
        assert res["ratio"] <= 1.0, (case, sig, "fmean", res["ratio"])
        assert not nc["wrong"], (case, sig, nc["wrong"][:4])
        assert nc["ratio"] <= 1.0 and not nc["unbounded"], (case, sig, "nccf", nc["ratio"])
    energy, vuv = g["energy"], g["vuv"].bool()
    cp, cm = g["cand"][:4], g["cand"][4:]
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
    ref_track = torch.from_numpy(fx[case.name][0])
    diff = (torch.nonzero(f0[1:] != ref_track[1:]).flatten() + 1).tolist()
    print(f"{case.name}: {nf} frames, frame 0 {'equal' if f0[0] == ref_track[0] else 'differs'}; off the reference's track: {diff[:8]}")
    # (tests/test_yaapt_wide_host.py lists no frame where the float32 oracle leaves the reference's track: none is excluded here)
    assert f0.shape == ref_track.shape and diff == []
    if case.name == ywc.NAN_ROW:
        assert bool(torch.isnan(pstd)) and bool(torch.isnan(g["tm"]).all())


def test_the_means_decide_on_the_70_hz_case():
    """the device's frame means are a sizeable part of the samples there, and the one-deep reading of them (the resident kernels') is
    more than 100 bounds away: what makes check 1 a check of the depth"""
    import ref64_yaapt as r64
    from oracle import yaapt as oy
    case = ywc.by_name(ywc.MEAN70)
    _, g = run(case)
    plan = oy.Plan(case.n, case.opts)
    x, fm = g["filt"][0].numpy(), g["fmean"][0].numpy()
    assert float(np.abs(fm).mean() / np.abs(x).mean()) > 0.05
    want, bound = r64.frame_means(x, fm, plan, DEVICE)               # mean[k - 1] on the first `ov` samples only
    assert float(np.max(np.abs(fm - want)[4:] / bound[4:])) > 100.0


# ---- 2: the raising case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ywc.raising(), ids=repr)
def test_raises_where_the_reference_does(case, gold):
    from satools_amd import f0 as f0_hip
    assert str(gold.npz("fx_f0_wide.npz")["raised/" + case.name]) == case.raises == "RuntimeError"
    f0, st = f0_hip.yaapt_long(case.wav().unsqueeze(0).to(DEV), case.opts, defer_status=True)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="no voiced frame"):
        st.check()
    assert st.words.tolist() == [1]
    with pytest.raises(RuntimeError, match="no voiced frame"):
        f0_hip.track(case.wav().unsqueeze(0).to(DEV), case.opts)


# ---- 3: chunks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ywc.accepted(), ids=repr)
def test_chunk_64_and_128_have_the_default_chunks_bits(case):
    wav = case.wav().unsqueeze(0)
    want = entry(wav, case.opts, long=True, chunk=0)
    assert want[0].shape == (1, case.nframes) and want[1].tolist() == [0]
    assert torch.equal(bits(want[0][0]), bits(run(case)[0]))                # and f0.yaapt_long is that call
    for chunk in (64, 128):
        assert_same_run(entry(wav, case.opts, long=True, chunk=chunk), want, (case, chunk))


# ---- 4: ragged -------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_of_defaults_rows_has_the_bits_of_the_single_calls():
    from satools_amd import f0 as f0_hip
    cases = [ywc.by_name(n) for n in (ywc.CHUNK_EDGE[0], ywc.BEYOND_RESIDENT, ywc.CHUNK_EDGE[1], ywc.NAN_ROW, ywc.MEAN70)]
    assert [c.nframes for c in cases] == [65, 2049, 129, 8, 128] and all(c.opts == {} for c in cases)
    n_max = max(c.n for c in cases)
    wav = torch.zeros(len(cases), n_max)
    for i, c in enumerate(cases):
        wav[i, :c.n] = c.wav()
    lens = [c.n for c in cases]
    got = f0_hip.yaapt_long(wav.to(DEV), {}, lengths=lens).cpu()
    also = f0_hip.track(wav.to(DEV), {}, lengths=lens).cpu()
    at64 = f0_hip.yaapt_long(wav.to(DEV), {}, lengths=lens, chunk_frames=64).cpu()
    assert got.shape == (len(cases), 2049) and torch.equal(bits(got), bits(also)) and torch.equal(bits(got), bits(at64))
    assert bool(torch.isnan(run(cases[3])[1]["tm"]).all())                 # the NaN row: every NCCF merit of it is NaN
    for i, c in enumerate(cases):
        one = run(c)[0]
        assert torch.equal(bits(got[i, :c.nframes]), bits(one)), (i, c, torch.nonzero(got[i, :c.nframes] != one).flatten()[:8].tolist())
        assert not got[i, c.nframes:].any(), (i, c)


# ---- 5: red zones ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,ragged", [("defaults", 20481, False), ("defaults", 20481, True), ("d7", 10241, False), ("d7", 10241, True)], ids=str)
def test_red_zones_around_every_buffer(name, n, ragged):
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    lib = _lib.lib()
    opts = ywc.wide_set(name).opts
    B, chunk = (2 if ragged else 1), 64
    P = f0_hip.make_plan(n, dict(opts))
    assert P.nframes == 129 and P.tda_len - P.frame_jump > 128
    wav = torch.stack([yc.noisy_tone(3 + b, n) for b in range(B)])
    lens = [n, n - 6000][:B]
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


# ---- 6: the refusal --------------------------------------------------------------------------------------------------------------------------
def test_eight_frames_deep_is_refused_by_name_with_nothing_launched():
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    lib = _lib.lib()
    s = ywc.wide_set("d8")
    case = s.cases[0]
    P = f0_hip.make_plan(case.n, dict(s.opts))
    hann, kaiser, tw = f0_hip._get_tables(P, torch.device(DEV))
    wav = case.wav().unsqueeze(0).to(DEV)
    nws = lib.sat_yaapt_long_workspace_bytes(C.byref(P), 1, 0)
    assert nws > 0                                                     # the size function is unchanged: it knows no depth
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    f0 = torch.full((1, P.nframes), -7.0, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    for dims in (None, torch.tensor([f0_hip.length_dims(P, case.n)], dtype=torch.int32, device=DEV)):
        rc = lib.sat_yaapt_long_f32(C.byref(P), p(wav), p(dims), p(f0), p(status), p(hann), p(kaiser), p(tw), p(ws), nws, 1, 0, _lib.stream())
        assert rc == -1                                                # SAT_ERR_INVALID
        with pytest.raises(_lib.SatError, match=s.refused):
            _lib.check(rc, "sat_yaapt_long_f32")
        torch.cuda.synchronize()
        assert bool((f0 == -7.0).all()) and status.tolist() == [-7] and not ws.any()
    for call in (lambda: f0_hip.yaapt_long(wav, s.opts), lambda: f0_hip.track(wav, s.opts), lambda: f0_hip.track(wav, s.opts, lengths=[case.n])):
        with pytest.raises(_lib.SatError, match=s.refused):
            call()
    # the resident forms keep their overlap requirement and its message
    with pytest.raises(_lib.SatError, match="tda_frame_length / frame_space combination not supported"):
        f0_hip.yaapt(wav, {})
    good = ywc.by_name(ywc.CHUNK_EDGE[0])
    again = f0_hip.yaapt_long(good.wav().unsqueeze(0).to(DEV), good.opts).cpu()
    torch.cuda.synchronize()
    assert torch.equal(bits(again[0]), bits(run(good)[0]))


# ---- 7: end to end ---------------------------------------------------------------------------------------------------------------------------
def test_get_f0_and_convert_with_the_references_default_options():
    from satools_amd import f0 as f0_hip
    from satools_amd import synthetic
    model = _model(FBANK_TAG)
    keep = model.f0_yaapt_opts
    wav = synthetic.harm_batch([0, 5], 16000)
    try:
        model.f0_yaapt_opts = {}
        want = f0_hip.yaapt_long(wav.to(DEV), {}).cpu()
        f0 = model.get_f0(wav.to(DEV)).cpu()
        assert f0.shape == want.shape == (2, 100) and torch.equal(bits(f0), bits(want)) and bool((f0 > 0).any())
        rag = model.get_f0_ragged(wav.to(DEV), [16000, 12000]).cpu()
        assert torch.equal(bits(rag[0]), bits(want[0])) and not rag[1, 75:].any()
        y = model.convert(wav.to(DEV), target=[model.spk[5], model.spk[7]]).cpu()
        assert y.dim() >= 2 and y.shape[0] == 2 and torch.isfinite(y).all() and float(y.abs().max()) > 0
    finally:
        model.f0_yaapt_opts = keep
    y20 = model.convert(wav.to(DEV), target=[model.spk[5], model.spk[7]]).cpu()          # and the model's own options still run
    assert y20.shape[0] == 2 and torch.isfinite(y20).all()
