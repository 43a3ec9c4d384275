"""The packed real-input FFT of yaapt_nlfer_kernel and yaapt_spec_kernel (csrc/yaapt.hip) on the device, at the frame lengths
and bin ranges where its load, its stage skipping and its untangle can go wrong.  Needs a real MI355X: run with `-m gpu`.

Per option set ONE `yaapt(..., return_aux=True)` call on two utterances of 8000 samples (25 frames): the catalogue's harmonic tone,
and a 120 Hz sine with a second harmonic at 1e-4 of it (bins far below the frame's strongest one: where a closed-form FFT bound
would hide an error and the running bound does not).  From the device's own `filt`:
  * `e_raw` against the float64 NLFER sum and its bound (tests/ref64_yaapt.judge_e_raw),
  * the candidates behind the SHC against the float64 peak list and merit bounds (judge_cand): pitches equal wherever the float64
    decision is certain, merits within the bound, as tests/test_hip_yaapt_stages.py does; a ratio above 1 fails.
Then: each row of the batch equals its single-utterance run bit for bit, and so does each row of a ragged batch whose second
utterance is shorter (sat_yaapt_ragged_f32 launches the same kernels).

The option sets:
  35 ms      frame 560 / 1120: the anonymizer's; packed lengths 280 / 560 (3 / 2 copy stages)
  32 ms      512 / 1024: packed lengths 256 and 512, the spectral frame exactly on the 3-copy-stage edge
  32.07 ms   513 / 1026: one sample pair past it (2 copy stages), the NLFER frame odd
  34.95 ms   559 / 1118: an odd frame, the last imaginary part zero
  40 ms      640 / 1280: the entry point's limit
  f0_min 19  min_shc = 10 = half_wl: the SHC window of the first row starts at magnitude index 10, bin 0 (the k = 0 form)
  f0_min 2   NLFER bins from 1 on (nl_lo = 1), and the SHC window over bin 0 again

ROUNDINGS read off the kernels: twiddle x node as before (table twiddle 1 U + four-multiply product sqrt 5 U = 3.24 -> cmul 3.25); the
untangle's E and O take one rounding each where a stage's a + wb takes one, the halving is exact, so the 12 stages and the untangle
are the 13 levels the running bound walks; hypotf 2 ULP budgeted; the NLFER sum keeps block_sum256's 256-thread order
(ceil(n / 256) adds per thread + 8); the spectral mean, the SHC sum and the peak-range mean are untouched kernels' or orders'.

MEASURED on an MI355X: `e_raw` at most 0.038 of its bound, the candidate merits 0.007, no exempt frame; 7 tests in 2.9 s."""
import math

import numpy as np
import pytest
import torch

import ref64_yaapt as r64
import yaapt_cases as yc

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 8000
_c = math.ceil
DEVICE = r64.Roundings(cmul=3.25, hyp=4, nl_sum=lambda n: _c(n / 256) + 8, en_mean=lambda n: _c(n / 256) + 8,
                       sp_mean=lambda n: _c(n / 256) + 9, shc_sum=lambda n: n, shc_avg=lambda n: _c(n / 256) + 8,
                       fm_head=None, fm_tail=None, dot=None, pw=None)


def weak_harmonic(n):
    """0.4 sin(2 pi 120 t) + 4e-5 sin(2 pi 240 t): float64, rounded once"""
    t = torch.arange(n, dtype=torch.float64) / yc.SR
    return (0.4 * torch.sin(2 * np.pi * 120.0 * t) + 0.4 * 1e-4 * torch.sin(2 * np.pi * 240.0 * t)).float()


def _o(**kw):
    return {**yc.OPTS, **{k: float(v) for k, v in kw.items()}}


# name -> (options, plan fields that put the set on its edge)
SETS = {
    "35ms": (_o(), dict(frame_size=560, nframe_size=1120)),
    "32ms": (_o(frame_length=32), dict(frame_size=512, nframe_size=1024)),
    "32.07ms": (_o(frame_length=32.07), dict(frame_size=513, nframe_size=1026)),
    "34.95ms": (_o(frame_length=34.95), dict(frame_size=559, nframe_size=1118)),
    "40ms": (_o(frame_length=40), dict(frame_size=640, nframe_size=1280)),
    "f0min19": (_o(f0_min=19), dict(min_shc=10, half_wl=10, nl_lo=18)),
    "f0min2": (_o(f0_min=2), dict(nl_lo=1, min_shc=2)),
}


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def signals():
    return torch.stack((yc.tone(N), weak_harmonic(N)))


def judge_row(filt, e_raw, vuv, cand, plan):
    """one utterance's float32 results (numpy) -> {stage: dict(ratio, exempt, wrong)}"""
    return {"e_raw": r64.judge_e_raw(filt[0], e_raw, plan, DEVICE),
            "cand": r64.judge_cand(filt[1], vuv, cand[:4], cand[4:], plan, DEVICE)}


def check_row(name, row, res, vuv):
    for stage, r in res.items():
        print(f"  {name} row {row} {stage:6s} error / bound {r['ratio']:8.4f}" + (f"   exempt {r['exempt']}" if r.get("exempt") else ""))
    for stage, r in res.items():
        assert not r.get("wrong"), (name, row, stage, r["wrong"][:4])
        assert r["ratio"] <= 1.0, (name, row, stage, r["ratio"])
    voiced = int(np.asarray(vuv).astype(bool).sum())
    assert voiced >= 10 and len(res["cand"]["exempt"]) < voiced, (name, row, voiced, res["cand"]["exempt"])   # the check is not vacuous


@pytest.mark.parametrize("name", list(SETS), ids=str)
def test_packed_fft_stages_and_rows(name):
    from oracle import yaapt as oy
    from satools_amd import f0 as f0_hip
    opts, fields = SETS[name]
    plan = oy.Plan(N, opts)
    for key, want in fields.items():
        assert getattr(plan, key) == want, (name, key, getattr(plan, key), want)
    wav = signals().to(DEV)
    f0, aux = f0_hip.yaapt(wav, opts, return_aux=True)
    f0 = f0.cpu()
    g = {k: aux[k].cpu().numpy() for k in ("filt", "e_raw", "vuv", "cand")}
    assert f0.shape == (2, plan.nframes) and plan.nframes == 25
    print()
    for row in range(2):
        res = judge_row(g["filt"][row], g["e_raw"][row], g["vuv"][row], g["cand"][row], plan)
        check_row(name, row, res, g["vuv"][row])
    # a batch row is its single-utterance run
    for row in range(2):
        one = f0_hip.yaapt(wav[row:row + 1], opts).cpu()[0]
        assert torch.equal(f0[row], one), (name, row, torch.nonzero(f0[row] != one).flatten()[:8].tolist())
    # ragged: the second utterance shorter, both rows their single-utterance runs, zero past the shorter one's frames
    n1 = 6400
    nf1 = oy.Plan(n1, opts).nframes
    rag = wav.clone()
    rag[1, n1:] = 0
    got = f0_hip.yaapt_ragged(rag, [N, n1], opts).cpu()
    short = f0_hip.yaapt(wav[1:2, :n1], opts).cpu()[0]
    assert nf1 < plan.nframes and short.shape == (nf1,)
    assert torch.equal(got[0], f0[0]), (name, "ragged row 0")
    assert torch.equal(got[1, :nf1], short), (name, "ragged row 1", torch.nonzero(got[1, :nf1] != short).flatten()[:8].tolist())
    assert not got[1, nf1:].any()
