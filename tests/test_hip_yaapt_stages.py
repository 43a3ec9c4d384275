"""YAAPT on the HIP device, STAGE BY STAGE, on the edge catalogue of tests/yaapt_cases.py: frame counts and voiced counts on
the lane edges (63 / 64 / 65, 127 .. 129, 255 .. 257 and the entry point's limits of 4 and 2048 frames), one, two and a few
frames with a spectral candidate (the NaN `pitch_std`, the constant-150-Hz branch, the smallest Viterbi), utterances the
reference raises on, noise rows with a NaN `mean_pitch`, a clipped tone.  Needs a real MI355X: run with `-m gpu`
(`-s` prints the largest error / bound ratio and the exempted frames of every stage).

Every accepted case is run ONCE with `return_aux=True` and each stage is checked FROM THE DEVICE'S OWN UPSTREAM
INTERMEDIATES, so a wrong stage is named and the stages after it are not blamed for it.

EXACT (torch.equal, NaN = NaN): `filt` against oracle/biquad.py with its zero extension; `vuv` against the device energy;
the default candidates of unvoiced frames; `spec_pitch` and `pitch_std` against oracle.spec_select(device candidates);
the six refined pitch and merit rows against oracle.refine(device tp, tm, spec_pitch, energy, vuv);
the final track against oracle.dynamic(oracle.refine(device tp, tm, spec_pitch, energy, vuv)) — all-NaN `tm` and a NaN
`mean_pitch` included —; the final track against the reference's own (tests/golden/fx_f0_edges.npz, frame 0 exempt as in
tests/test_hip_yaapt.py).

BOUNDED (float64 references and bounds of tests/ref64_yaapt.py, U = 2^-24): `e_raw`, `energy`, the SHC-derived candidate
merits, `fmean`, and `tm` at the lag the device chose.  The rounding counts are read off csrc/yaapt.hip (DEVICE below);
nothing is fitted to what the kernels return.  A ratio of observed error to bound above 1 fails.

DECISIONS float32 may flip — `vuv` against the float64 energy, the peak set behind the candidate pitches, the NCCF lag
behind `tp` — must equal the float64 decision wherever its margin clears the bound.  A frame inside the bound is exempt,
counted and listed: none may be on the gated-tone cases, at most 1 % of the frames on the noise and clipped cases.
Frames whose NCCF has NO finite bound (float32 underflow in the silence after a burst, tests/ref64_yaapt.py) are listed
apart; only the cases that declare `underflows` may have them, and only at definitely-unvoiced frames.

MEASURED on an MI355X (profiles/yaapt_stage_error_ratios.txt): every ratio <= 0.27, no exempt frame, 38 tests in 9 s.

MUTATION CHECK (scratch builds, not committed; recorded in the same file).  `tmax` -> `fmaxf` in the `pitch_std` line: the
three NaN-`pitch_std` cases turn red, tests/test_hip_yaapt.py stays green.  The NaN branch removed from `path1_takes`:
15 cases with a NaN `mean_pitch` turn red, tests/test_hip_yaapt.py stays green.  `(1ull << tid) - 1ull` -> `(1ull << tid)` in
`compact_frames`: every case it was run on turns red (run on the 64 .. 66-frame single calls only: the mutant reads the
candidates through an unwritten frame list, and only there do those reads stay inside the workspace).  `i += 64` ->
`i += 63` in `medfilt_par` is an equivalent mutant: the lanes then compute some medians twice, from a read-only input
into a separate output, so every output value is unchanged and no test can tell."""
import math
import os
import time

import numpy as np
import pytest
import torch

import ref64_yaapt as r64
import yaapt_cases as yc

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPTS = yc.OPTS

# ROUNDINGS OF THE KERNELS (csrc/yaapt.hip), per sum of n terms unless a plain count:
#   cmul     twiddle x node: table twiddle rounded once (1 U) + complex product (sqrt 5 U) = 3.24, rounded up
#   hyp      hypotf: 1 ULP = 2 U tabulated in the HIP math API, 2 ULP budgeted
#   nl_sum   block_sum256 over the bins: ceil(n / 256) adds per thread, six shuffle levels, (r0 + r1) + (r2 + r3)
#   en_mean  the same reduction over the frames (the two divisions are counted in ref64_yaapt.energy_norm)
#   sp_mean  window product 1, ceil(n / 256) adds per thread, 8 for the block reduction (the division is counted there)
#   shc_sum  the SHC window: n sequential adds (the harmonic products are counted there)
#   shc_avg  block_sum256 over the peak range
#   fm_head  x - previous mean 1, v0 + v1 1, six shuffle levels (two loads per lane whatever the overlap: it is at most 128);
#            fm_tail: ceil(n / 64) adds per lane, six shuffle levels, n = frame_jump
#   dot      the NCCF's four FMA accumulators: n // 4 fused steps each and the n % 4 left-over terms on the FIRST one (its tail loop),
#            then (n0 + n1) + (n2 + n3).  n = tda_len - lag_max follows the data, so n % 4 takes every value under any plan
#   pw       block_sum256 of d * d: product and add per term, ceil(n / 256) terms per thread, 8 for the reduction
_c = math.ceil
DEVICE = r64.Roundings(cmul=3.25, hyp=4, nl_sum=lambda n: _c(n / 256) + 8, en_mean=lambda n: _c(n / 256) + 8,
                       sp_mean=lambda n: _c(n / 256) + 9, shc_sum=lambda n: n, shc_avg=lambda n: _c(n / 256) + 8,
                       fm_head=lambda n: 8, fm_tail=lambda n: _c(n / 64) + 6, dot=lambda n: n // 4 + n % 4 + 2,
                       pw=lambda n: 2 * _c(n / 256) + 8)

_RATIOS, _EXEMPT, _T0 = {}, {}, time.time()
_RUNS = {}


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    """prints the largest error / bound ratio of every stage and the exempted frames when the module is done (and writes
    the table to the file SAT_YAAPT_STAGE_RATIOS names, if set)"""
    yield
    lines = [f"{k:12s} {r:8.4f}   at {case}" for k, (r, case) in sorted(_RATIOS.items())]
    lines.append("frames inside the float64 bound of a decision (exempt; `/unbounded`: no finite bound), per case and stage:"
                 + ("" if _EXEMPT else " none"))
    lines += [f"  {name}: {stages}" for name, stages in sorted(_EXEMPT.items())]
    lines.append(f"wall time of tests/test_hip_yaapt_stages.py: {time.time() - _T0:.1f} s")
    print("\nYAAPT stages: largest observed error / derived bound (a ratio above 1 fails)\n" + "\n".join(lines))
    path = os.environ.get("SAT_YAAPT_STAGE_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_yaapt_stages.py: largest observed error / derived bound, per stage (a ratio above 1 fails)\n")
            f.write("\n".join(lines) + "\n")


def device_run(case):
    """-> (f0 [nframes], {name: cpu tensor of utterance 0}) of ONE `yaapt(..., return_aux=True)` call, kept for the batch tests"""
    from satools_amd import f0 as f0_hip
    if case.name not in _RUNS:
        f0, aux = f0_hip.yaapt(case.wav().unsqueeze(0).to(DEV), case.opts, return_aux=True)
        _RUNS[case.name] = (f0.cpu()[0], {k: v.cpu()[0] for k, v in aux.items()})
    return _RUNS[case.name]


def same(a, b):
    """torch.equal with NaN equal to NaN"""
    a, b = torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _ranges(frames):
    """[3, 4, 5, 9] -> '3-5, 9'"""
    out, i = [], 0
    while i < len(frames):
        j = i
        while j + 1 < len(frames) and frames[j + 1] == frames[j] + 1:
            j += 1
        out.append(str(frames[i]) if i == j else f"{frames[i]}-{frames[j]}")
        i = j + 1
    return ", ".join(out)


def _note(stage, case, res, ratios=None, exempt=None, key=None):
    ratios, exempt = (_RATIOS if ratios is None else ratios), (_EXEMPT if exempt is None else exempt)
    r = res["ratio"]
    print(f"  {stage:10s} error / bound {r:8.4f}" + (f"   exempt {res['exempt']}" if res.get("exempt") else "")
          + (f"   unbounded {res['unbounded']}" if res.get("unbounded") else ""))
    if r > ratios.get(key or stage, (-1.0, ""))[0]:
        ratios[key or stage] = (r, case.name)
    for k in ("exempt", "unbounded"):
        if res.get(k):
            exempt.setdefault(case.name, {})[stage + ("" if k == "exempt" else "/unbounded")] = _ranges(res[k])


@pytest.mark.parametrize("case", yc.accepted(), ids=repr)
def test_every_stage_from_the_devices_own_upstream(case, gold):
    check_every_stage(case, gold.npz("fx_f0_edges.npz"))


def check_every_stage(case, fx, note=_note):
    """the stage checks of one accepted case under ITS option set (`case.opts`: the catalogue's cases carry OPTS, the (case, set) pairs
    of tests/test_hip_yaapt_options.py their set), against the reference tracks of the fixture `fx`"""
    from oracle import biquad
    from oracle import yaapt as oy
    plan = oy.Plan(case.n, case.opts)
    f0, g = device_run(case)
    nf = plan.nframes
    assert f0.shape == (nf,) and case.nframes == nf
    energy, vuv = g["energy"], g["vuv"].bool()
    cp, cm = g["cand"][:4], g["cand"][4:]
    spec, pstd = g["spec_pitch"], g["scal"][0]

    # ---- exact ----------------------------------------------------------------------------------------------------
    x = np.concatenate([np.zeros(plan.pad, np.float32), case.wav().numpy(), np.zeros(plan.pad, np.float32)])
    filt = g["filt"].numpy()
    for sig, v in ((0, x), (1, x * x)):
        ref = biquad.band_limit(v, int(plan.fs), plan.p["bp_low"], plan.p["bp_high"])
        assert np.array_equal(filt[sig, :plan.L], ref), ("filt", sig, int((filt[sig, :plan.L] != ref).sum()))
        assert not filt[sig, plan.L:].any(), ("filt zero extension", sig)
    assert torch.equal(vuv, energy > plan.p["nlfer_thresh1"]), "vuv"
    assert not cp[:, ~vuv].any() and bool((cm[:, ~vuv] == 1).all()), "default candidates of unvoiced frames"
    want_spec, want_std = oy.spec_select(cp.clone(), cm.clone(), plan)
    assert same(spec, want_spec), ("spec_pitch", torch.nonzero(spec != want_spec).flatten()[:8].tolist())
    assert same(pstd, want_std), ("pitch_std", float(pstd), float(want_std))
    z = torch.zeros(2, nf)
    tp1, tm1 = torch.cat((g["tp"][0:1], z)), torch.cat((g["tm"][0:1], z))
    tp2, tm2 = torch.cat((g["tp"][1:2], z)), torch.cat((g["tm"][1:2], z))
    rp, rm = oy.refine(tp1, tm1, tp2, tm2, spec.clone(), energy, vuv, plan)
    # refine() itself, row by row (the final track shows one row per frame; `merit_pivot`, for one, never shows in it: at a frame with
    # energy <= nlfer_thresh2 every row it fills has pitch 0)
    assert same(g["refined"][:6], rp), ("refined pitch", torch.nonzero(torch.nan_to_num(g["refined"][:6]) != torch.nan_to_num(rp))[:8].tolist())
    assert same(g["refined"][6:], rm), ("refined merit", torch.nonzero(torch.nan_to_num(g["refined"][6:]) != torch.nan_to_num(rm))[:8].tolist())
    want_f0 = oy.dynamic(rp, rm, energy, plan)
    assert same(f0, want_f0), ("final f0", torch.nonzero(f0 != want_f0).flatten()[:8].tolist())
    assert str(fx["raised/" + case.name]) == ""
    ref_track = torch.from_numpy(fx[case.name][0])
    assert torch.equal(f0[1:], ref_track[1:]), ("reference track", torch.nonzero(f0 != ref_track).flatten()[:8].tolist())

    # ---- the properties the case is in the catalogue for, from the device's own intermediates ----------------------------
    got = yc.check_properties(case, dict(energy=energy, vuv=vuv, cand_pitch=cp, pitch_std=pstd, ref_pitch=rp))
    print(f"\n{case.name}: {got}")
    if case.std_nan:
        assert bool(torch.isnan(g["tm"]).all()) and not g["tp"].any()          # every merit NaN, no candidate
    if case.exact_only:
        return

    # ---- bounded, and the decisions ----------------------------------------------------------------------------------
    aux, _, raised = yc.oracle_run(case)                                       # the float32 oracle keeps the same properties
    assert raised == "" and yc.check_properties(case, aux)
    res = {"e_raw": r64.judge_e_raw(filt[0], g["e_raw"].numpy(), plan, DEVICE),
           "energy": r64.judge_energy_norm(g["e_raw"].numpy(), energy.numpy(), DEVICE),
           "vuv": r64.judge_vuv(filt[0], energy.numpy(), vuv.numpy(), plan, DEVICE),
           "cand": r64.judge_cand(filt[1], vuv.numpy(), cp.numpy(), cm.numpy(), plan, DEVICE)}
    for sig in (0, 1):
        fm = g["fmean"][sig].numpy()
        res[f"fmean{sig + 1}"] = r64.judge_fmean(filt[sig], fm, plan, DEVICE)
        res[f"nccf{sig + 1}"] = r64.judge_nccf(filt[sig], fm, spec.numpy(), float(pstd), g["tp"][sig].numpy(),
                                              g["tm"][sig].numpy(), plan, DEVICE)
    for stage, r in res.items():
        note(stage, case, r)
    for stage, r in res.items():
        assert not r.get("wrong"), (stage, r["wrong"][:4])
        assert r["ratio"] <= 1.0, (stage, r["ratio"])
    yc.assert_exempt_cap(case, res, energy)


# ---- batches ---------------------------------------------------------------------------------------------------------
RAGGED_MIX = ["tone_1280", "tone_20160", "tone_20480", "tone_20481", "tone_41280", "burst260_at20220_of20480",
              "burst270_at8000_of20480"]        # 4, 63, 64, 65 and 129 frames, nv == 1 (NaN), nv == 2


@pytest.mark.parametrize("B", [len(RAGGED_MIX), 33])
def test_ragged_batch_rows_are_their_single_tracks(B):
    """zero past each row's frames, bit for bit the single-utterance track: NaN does not cross rows.  33 rows: a second
    prefilter block of 32 and (41280 + 1 pad sample) the unaligned row path"""
    from satools_amd import f0 as f0_hip
    cases = [yc.by_name(RAGGED_MIX[i % len(RAGGED_MIX)]) for i in range(B)]
    n_max = max(c.n for c in cases) + (1 if B == 33 else 0)
    wav = torch.zeros(B, n_max)
    for i, c in enumerate(cases):
        wav[i, :c.n] = c.wav()
    got = f0_hip.yaapt_ragged(wav.to(DEV), [c.n for c in cases], OPTS).cpu()
    assert got.shape == (B, math.ceil(n_max / 320))
    assert not torch.isnan(got).any()
    for i, c in enumerate(cases):
        one, _ = device_run(c)
        assert torch.equal(got[i, :c.nframes], one), (i, c, torch.nonzero(got[i, :c.nframes] != one).flatten()[:8].tolist())
        assert not got[i, c.nframes:].any(), (i, c)


def test_status_names_the_utterance_without_a_candidate_only():
    from satools_amd import f0 as f0_hip
    cases = [yc.by_name("tone_20480"), yc.by_name("burst60_at8000_of20480"), yc.by_name("burst270_at8000_of20480")]
    wav = torch.stack([c.wav() for c in cases]).to(DEV)
    f0, status = f0_hip.yaapt(wav, OPTS, defer_status=True)
    f0 = f0.cpu()
    for i in (0, 2):
        assert torch.equal(f0[i], device_run(cases[i])[0]), i
    with pytest.raises(RuntimeError) as e:
        status.check()
    assert "utterance(s) [1] " in str(e.value), str(e.value)


@pytest.mark.parametrize("case", yc.raising(), ids=repr)
def test_raises_where_the_reference_does(case, gold):
    from satools_amd import f0 as f0_hip
    assert str(gold.npz("fx_f0_edges.npz")["raised/" + case.name]) == case.raises == "RuntimeError"
    with pytest.raises(RuntimeError, match="no voiced frame"):
        f0_hip.yaapt(case.wav().unsqueeze(0).to(DEV), OPTS)


def test_refusals_leave_no_sticky_error(gold):
    from satools_amd import _lib
    from satools_amd import f0 as f0_hip
    for case in yc.refused():
        with pytest.raises(_lib.SatError, match=rf"yaapt: {case.nframes} frames not supported \(4\.\.2048"):
            f0_hip.yaapt(case.wav().unsqueeze(0).to(DEV), OPTS)
    small = yc.by_name("tone_1280")
    again = f0_hip.yaapt(small.wav().unsqueeze(0).to(DEV), OPTS).cpu()[0]
    torch.cuda.synchronize()
    assert torch.equal(again, device_run(small)[0])
    assert torch.equal(again[1:], torch.from_numpy(gold.npz("fx_f0_edges.npz")["tone_1280"][0])[1:])
