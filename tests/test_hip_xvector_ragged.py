"""Ragged batches of the ECAPA-TDNN x-vector extractor (csrc/ragged/, include/satools_hip_ragged.h; xvector.Net.extract_batch) on the HIP
device.  Needs a real MI355X: run with `-m gpu`.

(1) Every segment kernel against the row kernel it is the segment form of, per utterance, BIT FOR BIT (torch.equal): the input's gap columns
    (and the samples past an utterance's end) are NaN.  Frame counts 4, 63, 64, 65, 127, 128, 129, 257 in a shuffled order — below / at /
    above the 64 lanes of a wave and twice that — with C = 5 and 8 (a block of four waves ends inside a row of segments); the chain at
    lengths 7, 63, 64, 65, 128, 129, 193 around its 64- and 128-column centres, both centres forced, every (pieces, dilation) of the net and
    (3, 1), also against the float64 chain of tests/test_hip_xvector.py at its bar 5e-6 max(1, |ref|); the front end at 513, 640, 10079, 10080,
    10240 and 24123 samples (4, 5, 63, 64, 65, 151 frames).
(2) Red zones around every buffer of every entry point under both fills (tests/moat.py): ROWS / FAMILIES, which
    tests/test_xvector_ragged_host.py holds against the header and the sources.  Input gap columns are don't-care, output gap columns
    untouched — the InstanceNorm's aside, which are owned zeros; the int32 tables are index buffers.
(3) The net: six utterances of different lengths in one call, each row against oracle.xvector on the CPU (5e-6, the bar of
    test_xvector_matches_reference_and_oracle), against the one-utterance call (1e-6, the project's bar for batch versus single), the norm,
    the reversed order; the three fixture utterances against tests/golden/fx_xvector.npz.
(4) No leak between segments: an utterance of NaNs (or with one NaN / infinite sample) gives a NaN row and leaves every other row's bits alone.
(5) Refusals.  (6) asv_eval.test_metrics with batch_size 1 and 4 on a toy directory.
The largest error / bound of (1) and (3) is printed and, if SAT_XVECTOR_RAGGED_RATIOS names a file, written there
(profiles/xvector_ragged_error_ratios.txt).

MEASURED on an MI355X (profiles/xvector_ragged_error_ratios.txt): every segment kernel has its row kernel's bits on every segment | the chain
0.16 of its float64 bar | the net's rows 1.5-2.4e-7 from the oracle (bar 5e-6), 1.2e-7 from the reference's fixtures, and the SAME BITS as the
one-utterance calls and as the reversed batch (bar 1e-6) | test_metrics with batch_size 4: the same bits as with 1 | a broken utterance: its
row all NaN, no other row changes.  The file's tests take 4.2 s on the GPU."""
import functools
import json
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moat import Buf, run_case

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# every SAT_LAUNCH_CHECK string of csrc/ragged/ (tests/test_xvector_ragged_host.py holds this against the sources)
FAMILIES = ["melspec_logmel_segments_kernel", "instnorm_segments_kernel", "row_mean_segments_kernel", "se_gate_add_segments_kernel",
            "attentive_stats_segments_kernel", "res2_chain_segments_kernel"]
WAVE = 64                                                   # lanes of the strided reductions
FRAMES = (65, 4, 257, 63, 128, 64, 129, 127)                # shuffled
CHANNELS = (5, 8)
CHAIN_FRAMES = (64, 7, 193, 63, 129, 65, 128)               # shuffled
CHAIN_CASES = ((7, 2), (7, 3), (7, 4), (3, 1))              # (pieces, dilation)
CENTRES = (64, 128)
FRONT_SAMPLES = (10080, 513, 24123, 640, 10240, 10079)      # 64, 4, 151, 5, 65, 63 frames
NET_SAMPLES = (8000, 10079, 10080, 16000, 24123, 641)
FIXTURE_UTTERANCES = (("harm0_16000", 0, 16000), ("harm3_48000", 3, 48000), ("harm7_24123", 7, 24123))

_RATIOS = {}


def _note(name, r, what):
    if r > _RATIOS.get(name, (-1.0, ""))[0]:
        _RATIOS[name] = (r, what)


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    lines = [f"{k:52s} {r:10.4f}   at {what}" for k, (r, what) in sorted(_RATIOS.items())]
    print("\nlargest observed error / bound per quantity (0 = the same bits):\n" + "\n".join(lines))
    path = os.environ.get("SAT_XVECTOR_RAGGED_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_xvector_ragged.py: largest observed error / bound per quantity (a ratio above 1 fails; 0 = the same bits)\n")
            f.write("\n".join(lines) + "\n")


def _sat():
    import satools_amd  # noqa: F401
    from satools_amd import _lib, ops
    return _lib, ops


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def layout(frames):
    _, ops = _sat()
    off, length, t_tot = ops.ragged_layout(frames)
    return [int(o) for o in off], [int(n) for n in length], int(t_tot)


def gap_mask(frames, rows):
    """bool [rows, T_tot]: True on the columns outside every segment"""
    off, length, t_tot = layout(frames)
    m = torch.ones(rows, t_tot, dtype=torch.bool)
    for o, n in zip(off, length):
        m[:, o:o + n] = False
    return m


def pack(segments, frames, fill=float("nan")):
    """per-utterance CPU tensors [C, T_i] -> packed [C, T_tot] with `fill` in the gap columns"""
    off, length, t_tot = layout(frames)
    out = torch.full((segments[0].shape[0], t_tot), fill)
    for s, o, n in zip(segments, off, length):
        out[:, o:o + n] = s
    return out


@functools.lru_cache(maxsize=None)
def rows_case(C, which):
    """random per-utterance rows [C, T_i] for FRAMES (CPU, shared, never modified): an offset and a scale per (row, utterance)"""
    g = _gen(21, C, which)
    return tuple(torch.randn(C, t, generator=g) * (0.5 + i) + (i - 3.0) for i, t in enumerate(FRAMES))


def table(frames=None, n_samples=None):
    _, ops = _sat()
    return ops.RaggedTable(torch.device(DEV), n_samples=n_samples, frames=frames)


def _same(name, got, want, what):
    same = torch.equal(got, want)
    _note(name + " (bits)", 0.0 if same else float("inf"), what)
    assert same, (name, what, float((got - want).abs().max()))


# ---- (1) segment kernel = row kernel, bit for bit --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_instnorm_segments_is_the_row_kernel_per_segment_and_zero_in_the_gaps(C):
    _, ops = _sat()
    segs, tab = rows_case(C, 0), table(FRAMES)
    y = ops.instnorm_segments(pack(segs, FRAMES).to(DEV).unsqueeze(0), tab)
    assert y.shape == (1, C, tab.T_tot)
    for i, s in enumerate(segs):
        _same("instnorm_segments", tab.segment(y, i)[0], ops.instnorm_rows(s.to(DEV).unsqueeze(0))[0], f"C {C} segment {i} of {FRAMES[i]}")
    gaps = y[0].cpu()[gap_mask(FRAMES, C)]
    assert gaps.numel() == C * (tab.T_tot - sum(FRAMES)) and bool((gaps == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_row_mean_and_attentive_stats_segments_are_the_row_kernels_per_segment(C):
    _, ops = _sat()
    xs, ls, tab = rows_case(C, 1), rows_case(C, 2), table(FRAMES)
    x, lg = pack(xs, FRAMES).to(DEV), pack(ls, FRAMES).to(DEV)
    m = ops.row_mean_segments(x, tab)
    p = ops.attentive_stats_segments(x.unsqueeze(0), lg.unsqueeze(0), tab)
    assert m.shape == (len(FRAMES), C) and p.shape == (len(FRAMES), 2 * C)
    for i in range(len(FRAMES)):
        xi, li = xs[i].to(DEV).unsqueeze(0), ls[i].to(DEV).unsqueeze(0)
        _same("row_mean_segments", m[i], ops.row_mean(xi)[0, :, 0], f"C {C} segment {i} of {FRAMES[i]}")
        _same("attentive_stats_segments", p[i], ops.attentive_stats(xi, li)[0, :, 0], f"C {C} segment {i} of {FRAMES[i]}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("skips", [0, 1, 2, 3])
def test_se_gate_add_segments_is_the_row_kernel_per_segment_into_a_strided_slice(C, skips):
    _, ops = _sat()
    zs, tab = rows_case(C, 3), table(FRAMES)
    sk = [rows_case(C, 4 + k) for k in range(skips)]
    g = torch.randn(len(FRAMES), C, generator=_gen(22, C)).to(DEV)
    wide = torch.full((1, C + 3, tab.T_tot), -7.0, device=DEV)
    out = ops.se_gate_add_segments(pack(zs, FRAMES).to(DEV).unsqueeze(0), g, [pack(s, FRAMES).to(DEV).unsqueeze(0) for s in sk], tab, out=wide[:, 2:2 + C])
    assert out.data_ptr() == wide[:, 2:2 + C].data_ptr()
    for i in range(len(FRAMES)):
        want = ops.se_gate_add(zs[i].to(DEV).unsqueeze(0), g[i:i + 1], [s[i].to(DEV).unsqueeze(0) for s in sk])
        _same("se_gate_add_segments", tab.segment(out, i)[0], want[0], f"C {C} skips {skips} segment {i} of {FRAMES[i]}")
    w = wide[0].cpu()
    assert bool((w[:2] == -7.0).all()) and bool((w[2 + C:] == -7.0).all()) and bool((w[2:2 + C][gap_mask(FRAMES, C)] == -7.0).all())


@functools.lru_cache(maxsize=None)
def chain_case(nums, dil):
    """inputs of the chain for CHAIN_FRAMES and its float64 value per segment (the arithmetic of test_res2_chain_is_the_chain_of_convs)"""
    g = _gen(23, nums, dil)
    C = (nums + 1) * 64
    ys = tuple(torch.randn(C, t, generator=g) for t in CHAIN_FRAMES)
    w = torch.randn(nums, 64, 64, 3, generator=g) * (64 * 3) ** -0.5               # Conv1d.weight layout per piece: [co][ci][tap]
    sc, sh = torch.rand(nums, 64, generator=g) + 0.5, torch.randn(nums, 64, generator=g) * 0.1
    refs = []
    for y in ys:
        ref, sp = [], None
        for i in range(nums):
            xin = y[None, 64 * i:64 * (i + 1)].double() + (sp if sp is not None else 0)
            sp = F.conv1d(xin, w[i].double(), padding=dil, dilation=dil)
            sp = torch.relu(sp) * sc[i].double().view(1, -1, 1) + sh[i].double().view(1, -1, 1)
            ref.append(sp)
        ref.append(y[None, 64 * nums:].double())
        refs.append(torch.cat(ref, 1)[0])
    return dict(ys=ys, w=w.permute(0, 3, 2, 1).contiguous(), sc=sc, sh=sh, refs=tuple(refs), C=C)


@pytest.mark.gpu
@pytest.mark.parametrize("centre", CENTRES)
@pytest.mark.parametrize("nums,dil", CHAIN_CASES)
def test_res2_chain_segments_is_the_row_kernel_per_segment_and_the_float64_chain(nums, dil, centre):
    _lib, ops = _sat()
    c, tab = chain_case(nums, dil), table(CHAIN_FRAMES)
    w, sc, sh = c["w"].to(DEV), c["sc"].to(DEV), c["sh"].to(DEV)
    z = torch.full((1, c["C"], tab.T_tot), -7.0, device=DEV)
    ops.res2_chain_segments(pack(c["ys"], CHAIN_FRAMES).to(DEV).unsqueeze(0), w, sc, sh, dil, tab, centre=centre, out=z)
    assert _lib.lib().sat_last_dispatch_name().decode().split("<")[0].strip() == "res2_chain_segments_kernel"
    for i, y in enumerate(c["ys"]):
        what = f"pieces {nums} dilation {dil} centre {centre} segment {i} of {CHAIN_FRAMES[i]}"
        got = tab.segment(z, i)[0]
        _same("res2_chain_segments", got, ops.res2_chain(y.to(DEV).unsqueeze(0), w, sc, sh, dil)[0], what)
        ref = c["refs"][i]
        r = float((got.cpu().double() - ref).abs().max()) / (5e-6 * max(1.0, float(ref.abs().max())))
        _note("res2_chain_segments vs float64 / 5e-6 max(1, |ref|)", r, what)
        assert r < 1.0, (what, r)
    assert bool((z[0].cpu()[gap_mask(CHAIN_FRAMES, c["C"])] == -7.0).all())


@pytest.mark.gpu
def test_res2_chain_segments_automatic_centre_with_many_short_segments():
    """256 segments of 5 frames are 256 tiles of 128-column centres: centre = 0 takes the wide instantiation; 255 stay on the narrow one; both give
    the bits of either forced centre, and B = 256 segments sit in one row of blocks"""
    _, ops = _sat()
    g = _gen(24)
    w = (torch.randn(3, 3, 64, 64, generator=g) * (64 * 3) ** -0.5).to(DEV)
    sc, sh = (torch.rand(3, 64, generator=g) + 0.5).to(DEV), (torch.randn(3, 64, generator=g) * 0.1).to(DEV)
    for B in (256, 255):
        tab = table([5] * B)
        assert tab.n_tiles128 == B and tab.n_tiles64 == B and tab.T_tot == 8 * B
        y = torch.randn(1, 256, tab.T_tot, generator=g).to(DEV)
        z = {c: ops.res2_chain_segments(y, w, sc, sh, 1, tab, centre=c, out=torch.full_like(y, -7.0)) for c in (0, 64, 128)}
        assert torch.equal(z[0], z[64]) and torch.equal(z[0], z[128])
        _same("res2_chain_segments", tab.segment(z[0], B - 1)[0], ops.res2_chain(tab.segment(y, B - 1).contiguous(), w, sc, sh, 1)[0], f"{B} segments of 5, automatic centre")
        assert bool((z[0][0, :, 5:8] == -7.0).all())


def test_the_automatic_centre_follows_the_row_kernels_rule():
    """sum ceil(T_i / 128) >= 256 picks the 128-column centres: held on the table the entry point is given (no GPU)"""
    _, ops = _sat()
    assert ops.ragged_tiles([128] * 255 + [1])[2] == 256 and ops.ragged_tiles([129] * 127 + [1])[2] == 255


@functools.lru_cache(maxsize=None)
def front_case():
    from satools_amd import synthetic, xvector
    wavs = tuple(synthetic.harm_batch([3 + i], n)[0] for i, n in enumerate(FRONT_SAMPLES))
    padded = torch.full((len(wavs), max(FRONT_SAMPLES)), float("nan"))
    for i, w in enumerate(wavs):
        padded[i, :w.shape[0]] = w
    return dict(wavs=wavs, padded=padded, window=torch.hann_window(400, periodic=True), fb=xvector.mel_filterbank().t().contiguous())


@pytest.mark.gpu
def test_melspec_logmel_segments_is_the_row_kernel_per_utterance():
    _, ops = _sat()
    c, tab = front_case(), table(n_samples=FRONT_SAMPLES)
    assert tab.frames == [64, 4, 151, 5, 65, 63]
    window, fb = c["window"].to(DEV), c["fb"].to(DEV)
    out = torch.full((1, 80, tab.T_tot), -7.0, device=DEV)
    got = ops.melspec_logmel_segments(c["padded"].to(DEV), tab, window, fb, 0.97)
    assert got.shape == out.shape
    for i, w in enumerate(c["wavs"]):
        _same("melspec_logmel_segments", tab.segment(got, i)[0], ops.melspec_logmel(w.to(DEV).unsqueeze(0), window, fb, 0.97)[0],
              f"utterance {i} of {FRONT_SAMPLES[i]} samples")


# ---- (2) red zones (tests/moat.py) -----------------------------------------------------------------------------------------------
@dataclass
class Row:
    entry: str                   # the C-ABI function
    name: str
    shapes: list
    make: object                 # make(*shape) -> (specs, call, ref)  (runs on the GPU box only)


ROWS = []


def _tables(frames, n_samples=None):
    """the int32 tables as index buffers"""
    _, ops = _sat()
    off, length, t_tot = ops.ragged_layout(frames)
    tiles, n64, n128 = ops.ragged_tiles(frames)
    specs = [Buf("seg_off", "in", off.shape, torch.int32, data=torch.from_numpy(off.copy()), index=True),
             Buf("seg_len", "in", length.shape, torch.int32, data=torch.from_numpy(length.copy()), index=True)]
    return specs, tiles, n64, n128, int(t_tot)


def _family(_lib, name):
    assert _lib.lib().sat_last_dispatch_name().decode().split("<")[0].strip() == name


def _rows_bounds(kind, C):
    _lib, ops = _sat()
    B = len(FRAMES)
    tabs, _, _, _, T = _tables(FRAMES)
    gap = gap_mask(FRAMES, C)
    x = pack(rows_case(C, 1), FRAMES, 0.0)
    P = lambda t, n: t[n].data_ptr()
    if kind == "instnorm":
        specs = tabs + [Buf("x", "in", (C, T), data=x, dontcare=gap), Buf("y", "out", (C, T))]

        def call(t):
            _lib.check(_lib.lib().sat_instnorm_segments_f32(P(t, "x"), P(t, "y"), P(t, "seg_off"), P(t, "seg_len"), C, B, T, 1e-5, _lib.stream()), kind)
            _family(_lib, "instnorm_segments_kernel")

        def ref(t):
            y = t["y"].cpu()
            assert bool((y[gap] == 0).all())
            for i, s in enumerate(rows_case(C, 1)):
                assert torch.equal(y[:, layout(FRAMES)[0][i]:][:, :FRAMES[i]], ops.instnorm_rows(s.to(DEV).unsqueeze(0))[0].cpu())
    elif kind == "row_mean":
        specs = tabs + [Buf("x", "in", (C, T), data=x, dontcare=gap), Buf("y", "out", (B, C))]

        def call(t):
            _lib.check(_lib.lib().sat_row_mean_segments_f32(P(t, "x"), P(t, "y"), P(t, "seg_off"), P(t, "seg_len"), C, B, T, _lib.stream()), kind)
            _family(_lib, "row_mean_segments_kernel")

        def ref(t):
            for i, s in enumerate(rows_case(C, 1)):
                assert torch.equal(t["y"][i], ops.row_mean(s.to(DEV).unsqueeze(0))[0, :, 0])
    elif kind == "attentive_stats":
        lg = pack(rows_case(C, 2), FRAMES, 0.0)
        specs = tabs + [Buf("x", "in", (C, T), data=x, dontcare=gap), Buf("logits", "in", (C, T), data=lg, dontcare=gap), Buf("out", "out", (B, 2 * C))]

        def call(t):
            _lib.check(_lib.lib().sat_attentive_stats_segments_f32(P(t, "x"), P(t, "logits"), P(t, "out"), P(t, "seg_off"), P(t, "seg_len"), C, B, T,
                                                                   _lib.stream()), kind)
            _family(_lib, "attentive_stats_segments_kernel")

        def ref(t):
            for i in range(B):
                want = ops.attentive_stats(rows_case(C, 1)[i].to(DEV).unsqueeze(0), rows_case(C, 2)[i].to(DEV).unsqueeze(0))[0, :, 0]
                assert torch.equal(t["out"][i], want)
    else:
        raise AssertionError(kind)
    return specs, call, ref


def _gate_bounds(C, skips):
    """y: rows 2 .. 2 + C - 1 of a [C + 3][T_tot + 12] buffer, the first T_tot columns of each — a channel slice with a pitch of its own"""
    _lib, ops = _sat()
    B = len(FRAMES)
    tabs, _, _, _, T = _tables(FRAMES)
    gap = gap_mask(FRAMES, C)
    pitch = T + 12
    untouched = torch.ones(C + 3, pitch, dtype=torch.bool)
    untouched[2:2 + C, :T] = gap
    g = torch.randn(B, C, generator=_gen(22, C))
    specs = tabs + [Buf("z", "in", (C, T), data=pack(rows_case(C, 3), FRAMES, 0.0), dontcare=gap), Buf("g", "in", (B, C), data=g),
                    Buf("y", "out", (C + 3, pitch), untouched=untouched)]
    for k in range(skips):
        specs.append(Buf(f"s{k + 1}", "in", (C, T), data=pack(rows_case(C, 4 + k), FRAMES, 0.0), dontcare=gap))

    def call(t):
        P = lambda n: t[n].data_ptr() if n in t else None
        _lib.check(_lib.lib().sat_se_gate_add_segments_f32(P("z"), P("g"), P("s1"), P("s2"), P("s3"), t["y"][2:].data_ptr(), P("seg_off"), P("seg_len"), C, B,
                                                           T, pitch, _lib.stream()), "se_gate_add")
        _family(_lib, "se_gate_add_segments_kernel")

    def ref(t):
        off = layout(FRAMES)[0]
        for i in range(B):
            want = ops.se_gate_add(rows_case(C, 3)[i].to(DEV).unsqueeze(0), g[i:i + 1].to(DEV), [rows_case(C, 4 + k)[i].to(DEV).unsqueeze(0) for k in range(skips)])
            assert torch.equal(t["y"][2:2 + C, off[i]:off[i] + FRAMES[i]], want[0])
    return specs, call, ref


def _chain_bounds(nums, dil, centre):
    _lib, ops = _sat()
    c = chain_case(nums, dil)
    B, C = len(CHAIN_FRAMES), c["C"]
    tabs, tiles, n64, n128, T = _tables(CHAIN_FRAMES)
    gap = gap_mask(CHAIN_FRAMES, C)
    specs = tabs + [Buf("tiles", "in", tiles.shape, torch.int32, data=torch.from_numpy(tiles.copy()), index=True),
                    Buf("y", "in", (C, T), data=pack(c["ys"], CHAIN_FRAMES, 0.0), dontcare=gap), Buf("z", "out", (C, T), untouched=gap),
                    Buf("w", "in", c["w"].shape, data=c["w"]), Buf("scale", "in", (nums, 64), data=c["sc"]), Buf("shift", "in", (nums, 64), data=c["sh"])]

    def call(t):
        P = lambda n: t[n].data_ptr()
        _lib.check(_lib.lib().sat_res2_chain_segments_f32(P("y"), P("z"), P("w"), P("scale"), P("shift"), P("seg_off"), P("seg_len"), P("tiles"), n64, n128,
                                                          B, C, T, nums, dil, centre, _lib.stream()), "res2_chain_segments")
        _family(_lib, "res2_chain_segments_kernel")

    def ref(t):
        off = layout(CHAIN_FRAMES)[0]
        for i, r in enumerate(c["refs"]):
            got = t["z"][:, off[i]:off[i] + CHAIN_FRAMES[i]].cpu().double()
            assert float((got - r).abs().max()) < 5e-6 * max(1.0, float(r.abs().max()))
    return specs, call, ref


def _front_bounds():
    import ctypes
    _lib, ops = _sat()
    c = front_case()
    B, n_max = c["padded"].shape
    frames = [1 + n // 160 for n in FRONT_SAMPLES]
    tabs, _, _, _, T = _tables(frames)
    past = torch.arange(n_max).unsqueeze(0) >= torch.tensor(FRONT_SAMPLES).unsqueeze(1)
    nz = c["fb"] > 0
    lo = nz.float().argmax(1).to(torch.int32)
    hi = (513 - torch.flip(nz, [1]).float().argmax(1)).to(torch.int32)
    host = (ctypes.c_int32 * B)(*FRONT_SAMPLES)
    specs = tabs + [Buf("n_samples", "in", (B,), torch.int32, data=torch.tensor(FRONT_SAMPLES, dtype=torch.int32), index=True),
                    Buf("wav", "in", (B, n_max), data=torch.nan_to_num(c["padded"]), dontcare=past), Buf("out", "out", (80, T), untouched=gap_mask(frames, 80)),
                    Buf("window", "in", (400,), data=c["window"]), Buf("fb", "in", (80, 513), data=c["fb"]),
                    Buf("fb_lo", "in", (80,), torch.int32, data=lo, index=True), Buf("fb_hi", "in", (80,), torch.int32, data=hi, index=True)]

    def call(t):
        P = lambda n: t[n].data_ptr()
        _lib.check(_lib.lib().sat_melspec_logmel_segments_f32(P("wav"), P("n_samples"), host, P("seg_off"), P("seg_len"), P("out"), P("window"), P("fb"),
                                                              P("fb_lo"), P("fb_hi"), B, n_max, T, 80, 0.97, _lib.stream()), "melspec_logmel_segments")
        _family(_lib, "melspec_logmel_segments_kernel")

    def ref(t):
        off = layout(frames)[0]
        for i, w in enumerate(c["wavs"]):
            want = ops.melspec_logmel(w.to(DEV).unsqueeze(0), c["window"].to(DEV), c["fb"].to(DEV), 0.97)[0]
            assert torch.equal(t["out"][:, off[i]:off[i] + frames[i]], want)
    return specs, call, ref


ROWS.append(Row("sat_melspec_logmel_segments_f32", "front end", [()], _front_bounds))
ROWS.append(Row("sat_instnorm_segments_f32", "rows", [("instnorm", C) for C in CHANNELS], _rows_bounds))
ROWS.append(Row("sat_row_mean_segments_f32", "rows", [("row_mean", C) for C in CHANNELS], _rows_bounds))
ROWS.append(Row("sat_attentive_stats_segments_f32", "rows", [("attentive_stats", C) for C in CHANNELS], _rows_bounds))
ROWS.append(Row("sat_se_gate_add_segments_f32", "gate", [(C, k) for C in CHANNELS for k in (0, 1, 2, 3)], _gate_bounds))
ROWS.append(Row("sat_res2_chain_segments_f32", "chain", [(n, d, c) for n, d in CHAIN_CASES for c in CENTRES], _chain_bounds))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [(r, s) for r in ROWS for s in r.shapes], ids=lambda p: f"{p[0].entry[4:]}:{p[0].name}-" + "x".join(str(v) for v in p[1]))
def test_no_access_outside_the_buffers(p):
    r, shape = p
    specs, call, ref = r.make(*shape)
    v, m, plain = run_case(specs, call, DEV, sync=torch.cuda.synchronize)
    assert not v, f"{r.entry} [{r.name}] {shape}:\n" + "\n".join(str(x) for x in v)
    ref(m.t)


# ---- (3) the net -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    import satools_amd  # noqa: F401
    from satools_amd import synthetic, xvector
    m = xvector.build()(num_speakers=10)
    m.load_state_dict(synthetic.xvector_state(0, 10), strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def net_wavs():
    from satools_amd import synthetic
    return tuple(synthetic.harm_batch([10 + i], n)[0] for i, n in enumerate(NET_SAMPLES))


@pytest.fixture(scope="module")
def clean_rows(net):
    return net.extract_batch([w.to(DEV) for w in net_wavs()])


@pytest.mark.gpu
def test_ragged_batch_matches_the_oracle_the_single_calls_and_its_reversed_order(net, clean_rows):
    from oracle import xvector as ox
    from satools_amd import synthetic
    sd = synthetic.xvector_state(0, 10)
    wavs = net_wavs()
    assert clean_rows.shape == (len(wavs), 192)
    back = net.extract_batch([w.to(DEV) for w in reversed(wavs)])
    for i, w in enumerate(wavs):
        got = clean_rows[i].cpu()
        what = f"utterance {i} of {NET_SAMPLES[i]} samples"
        err = float((got - ox.xvector(sd, w.unsqueeze(0))[0]).abs().max())
        one = float((clean_rows[i] - net(w.to(DEV))[1][0]).abs().max())
        rev = float((clean_rows[i] - back[len(wavs) - 1 - i]).abs().max())
        nrm = abs(float(got.double().norm()) - 1.0)
        print(f"{what}: vs oracle {err:.2e}, vs the one-utterance call {one:.2e}, vs the reversed batch {rev:.2e}, | norm - 1 | {nrm:.2e}")
        _note("net row vs oracle / 5e-6", err / 5e-6, what)
        _note("net row vs one-utterance call / 1e-6", one / 1e-6, what)
        _note("net row vs reversed order / 1e-6", rev / 1e-6, what)
        _note("net | norm - 1 | / 1e-5", nrm / 1e-5, what)
        assert err < 5e-6 and one < 1e-6 and rev < 1e-6 and nrm < 1e-5, what


@pytest.mark.gpu
def test_the_fixture_utterances_in_one_ragged_call_match_the_reference(net):
    from satools_amd import synthetic
    fx = np.load(os.path.join(GOLD, "fx_xvector.npz"))
    wavs = [synthetic.harm_batch([seed], n)[0] for _, seed, n in FIXTURE_UTTERANCES]
    padded = torch.full((3, 48000), float("nan"))
    for i, w in enumerate(wavs):
        padded[i, :w.shape[0]] = w
    rows = net.extract_batch((padded.to(DEV), [n for _, _, n in FIXTURE_UTTERANCES]))     # the padded form of the argument, NaN past each end
    assert torch.equal(rows, net.extract_batch([w.to(DEV) for w in wavs]))
    for i, (tag, _, _) in enumerate(FIXTURE_UTTERANCES):
        got, ref = rows[i].cpu().numpy(), fx[tag + "/xvector"][0]
        err, cos = float(np.abs(got - ref).max()), float((got * ref).sum())
        print(f"{tag}: ragged row max abs error vs reference {err:.2e}, cosine {cos:.7f}")
        _note("net row vs reference fixture / 5e-6", err / 5e-6, tag)
        assert err < 5e-6 and cos > 0.999999 and abs(float(np.linalg.norm(got)) - 1.0) < 1e-5


# ---- (4) no leak between segments ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bad", [2, 1])
@pytest.mark.parametrize("how", ["all NaN", "one NaN sample", "one infinite sample"])
def test_a_broken_utterance_gives_a_nan_row_and_changes_no_other_rows_bits(net, bad, how):
    """layout and dispatch are identical in the two calls and no output column may depend on another segment or on a gap: every other row keeps
    its bits.  The broken utterance's own row is NaN: its whole feature segment is (the InstanceNorm's mean), and extract_batch carries that
    past the ReLUs of the conv epilogues, which are max(v, 0) and give 0 for NaN"""
    _, ops = _sat()
    wavs = [net_wavs()[i].to(DEV) for i in (1, 3, 5)]                             # 10079, 16000 and 641 samples
    dirty = list(wavs)
    if how == "all NaN":
        dirty[bad] = torch.full_like(wavs[bad], float("nan"))
    else:
        dirty[bad] = wavs[bad].clone()
        dirty[bad][333] = float("nan") if "NaN" in how else float("inf")
    clean, rows = net.extract_batch(wavs), net.extract_batch(dirty)
    assert bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(rows[bad]).all())
    for i in range(3):
        if i != bad:
            assert torch.equal(rows[i], clean[i]), i
    W = net._prepare(torch.device(DEV))
    tab = table(n_samples=[int(w.shape[0]) for w in dirty])
    mel = ops.melspec_logmel_segments(torch.nn.utils.rnn.pad_sequence(dirty, batch_first=True), tab, W["window"], W["fb"], W["coef"])
    feats = ops.instnorm_segments(mel, tab)
    assert bool(torch.isnan(tab.segment(feats, bad)).all())
    for i in range(3):
        if i != bad:
            assert bool(torch.isfinite(tab.segment(feats, i)).all())


# ---- (5) refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_extract_batch_refusals(net):
    from satools_amd._lib import SatError
    ok = net_wavs()[0].to(DEV)
    with pytest.raises(SatError, match=r"utterance 1 of 512 samples"):
        net.extract_batch([ok, ok[:512], ok])
    with pytest.raises(SatError, match=r"utterance 2 of 512 samples"):
        net.extract_batch((torch.zeros(3, 8000, device=DEV), [8000, 513, 512]))
    try:
        net.res2_chain = False
        with pytest.raises(SatError, match="fused Res2Net chain"):
            net.extract_batch([ok])
    finally:
        net.res2_chain = True
    with pytest.raises(SatError, match="1025 utterances"):
        net.extract_batch([ok[:600]] * 1025)
    with pytest.raises(SatError, match="no CPU fallback"):
        net.extract_batch([ok, ok.cpu()])
    with pytest.raises(SatError):
        net.extract_batch([])
    assert net.extract_batch([ok]).shape == (1, 192)                              # no sticky error


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    import ctypes
    _lib, ops = _sat()
    L = _lib.lib()
    tab = table(CHAIN_FRAMES)
    c = chain_case(3, 1)
    y = pack(c["ys"], CHAIN_FRAMES, 0.0).to(DEV)
    z = torch.full_like(y, -7.0)
    w, sc, sh = c["w"].to(DEV), c["sc"].to(DEV), c["sh"].to(DEV)
    P = lambda t: t.data_ptr()
    good = dict(y=P(y), z=P(z), off=P(tab.seg_off), tiles=P(tab.tiles), n64=tab.n_tiles64, n128=tab.n_tiles128, B=tab.B, C=256, T=tab.T_tot, nums=3, dil=1, centre=0)
    bad = {"null y": dict(y=None), "z aliases y": dict(z=P(y)), "null table": dict(off=None), "null tiles": dict(tiles=None), "B = 0": dict(B=0),
           "B = 1025": dict(B=1025), "T_tot = 0": dict(T=0), "C of another piece count": dict(C=512), "dilation 5": dict(dil=5), "dilation 0": dict(dil=0),
           "centre 32": dict(centre=32), "no 128-column tile": dict(centre=128, n128=0), "no 64-column tile": dict(n64=0), "negative tiles": dict(n64=-1)}
    for what, change in bad.items():
        a = dict(good, **change)
        st = L.sat_res2_chain_segments_f32(a["y"], a["z"], P(w), P(sc), P(sh), a["off"], P(tab.seg_len), a["tiles"], a["n64"], a["n128"], a["B"], a["C"], a["T"],
                                           a["nums"], a["dil"], a["centre"], _lib.stream())
        assert st == -1 and b"res2_chain_segments" in L.sat_last_error(), (what, st, L.sat_last_error())
    assert L.sat_res2_chain_segments_f32(P(y), P(z), P(w), P(sc), P(sh), P(tab.seg_off), P(tab.seg_len), P(tab.tiles), tab.n_tiles64, tab.n_tiles128, tab.B, 512,
                                         tab.T_tot, 7, 5, 0, _lib.stream()) == -1      # 7 x 5 > 32
    fc = front_case()
    ft = table(n_samples=FRONT_SAMPLES)
    out = torch.full((80, ft.T_tot), -7.0, device=DEV)
    wav, window, fb = fc["padded"].to(DEV), fc["window"].to(DEV), fc["fb"].to(DEV)
    lo, hi = ops.mel_filter_ranges(fb)
    short = (ctypes.c_int32 * 6)(10080, 513, 24123, 512, 10240, 10079)
    st = L.sat_melspec_logmel_segments_f32(P(wav), P(ft.n_samples), short, P(ft.seg_off), P(ft.seg_len), P(out), P(window), P(fb), P(lo), P(hi), 6, wav.shape[1],
                                           ft.T_tot, 80, 0.97, _lib.stream())
    assert st == -1 and b"utterance 3 of 512 samples" in L.sat_last_error(), L.sat_last_error()
    for name, args in (("instnorm_segments", (None, P(out), P(ft.seg_off), P(ft.seg_len), 80, 6, ft.T_tot, 1e-5)),
                       ("row_mean_segments", (P(out), P(out), P(ft.seg_off), None, 80, 6, ft.T_tot)),
                       ("attentive_stats_segments", (P(out), P(out), P(out), P(ft.seg_off), P(ft.seg_len), 80, 1025, ft.T_tot)),
                       ("se_gate_add_segments", (P(out), P(out), None, P(out), None, P(out), P(ft.seg_off), P(ft.seg_len), 80, 6, ft.T_tot, ft.T_tot))):
        assert getattr(L, f"sat_{name}_f32")(*args, _lib.stream()) == -1 and name.encode() in L.sat_last_error(), name
    torch.cuda.synchronize()
    assert bool((z == -7.0).all()) and bool((out == -7.0).all())                  # nothing ran


# ---- (6) test_metrics on a toy directory -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_test_metrics_in_ragged_batches_on_a_toy_directory(tmp_path):
    import satools_amd
    from satools_amd import asv_eval, pipeline, synthetic
    wavs = tmp_path / "wav"
    wavs.mkdir()
    enroll = {"spkA-u1": 0, "spkA-u2": 1, "spkB-u1": 2, "spkC-u1": 3}
    trial = {"spkA-u2": 1, "spkB-t1": 4, "spkC-t1": 5}                            # six files, one of both lists
    for name, seed in {**enroll, **trial}.items():
        pipeline.save_pcm16(wavs / (name + ".wav"), synthetic.harm_utterance(seed, 9000 + 2401 * seed).unsqueeze(0), 16000)
    (tmp_path / "enroll.scp").write_text("".join(f"{n} {wavs / (n + '.wav')}\n" for n in enroll))
    (tmp_path / "trials.scp").write_text("".join(f"{n} {wavs / (n + '.wav')}\n" for n in trial))
    (tmp_path / "utt2spk").write_text("".join(f"{n} {n.split('-')[0]}\n" for n in enroll))
    (tmp_path / "trials").write_text("".join(f"{s} {u} {'target' if u.startswith(s) else 'nontarget'}\n" for s in ("spkA", "spkB", "spkC") for u in trial))
    model = satools_amd.load_model("synthetic:xvector?speakers=12").to(DEV)
    seen = []
    inner = model.extract_batch
    model.extract_batch = lambda w: seen.append(len(w)) or inner(w)
    args = [str(tmp_path / n) for n in ("enroll.scp", "trials.scp", "utt2spk", "trials")]
    asv_eval.test_metrics(model, *args, str(tmp_path / "one"))
    assert seen == []
    asv_eval.test_metrics(model, *args, str(tmp_path / "four"), batch_size=4)
    assert seen == [4, 2]
    a, b = np.load(tmp_path / "one" / "xvectors.npz"), np.load(tmp_path / "four" / "xvectors.npz")
    assert a["utts"].tolist() == b["utts"].tolist() == list(enroll) + [u for u in trial if u not in enroll]
    d = float(np.abs(a["xvectors"] - b["xvectors"]).max())
    _note("test_metrics x-vectors, batch_size 4 vs 1 / 1e-6", d / 1e-6, "toy directory")
    assert d < 1e-6
    ma, mb = json.load(open(tmp_path / "one" / "metric.json")), json.load(open(tmp_path / "four" / "metric.json"))
    assert set(ma) == set(mb) and set(ma["asnorm"]) == set(mb["asnorm"])
    assert [l.split()[:2] for l in open(tmp_path / "one" / "scores")] == [l.split()[:2] for l in open(tmp_path / "four" / "scores")]
