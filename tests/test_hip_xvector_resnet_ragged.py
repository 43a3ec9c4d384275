"""Ragged batches of the ResNet x-vector extractor (csrc/ragged2d/, include/satools_hip_ragged2d.h; xvector_resnet.Net.extract_batch) on the
HIP device.  Needs a real MI355X: run with `-m gpu`.

(1) Every segment kernel against the kernel it is the segment form of, per utterance, BIT FOR BIT (torch.equal), with NaN in every input gap
    column.  Conv: widths 1, 2, 31, 32, 33, 63, 64, 65, 97 in a shuffled order (the 32-column tile at stride 1, and at stride 2 through
    Wo = 32 / 32 / 33), H = 5 (two row tiles, one row in the second; Ho = 3 at stride 2), every (Cin -> Cout, k, s) of CONVS — 256 -> 256 on
    three of the widths — under the epilogues none / affine / affine + ReLU, and one case whose output table has the segments in reverse
    order.  Plane mean: H T_i of 63, 64, 65, 128 and 129 elements (over H in {1, 5, 10} those counts factor with H = 1 only, so the 128 and
    129 are T_i = 128 and 129; every other T_i is 1 .. 65), C = 5 and 8.  Mean / deviation: lengths 2, 3, 63, 64, 65, 129.  SE tail: the conv's
    widths, H = 5.
(2) The conv cases of (1) against tests/ref64_resnet.conv2d per utterance, under the derived bound of
    test_hip_xvector_resnet.test_conv2d_against_float64:
        |err| <= (9 Cin + 4) U sum|w x| |scale|  +  U |sum scale|  +  U |sum scale + shift|,   U = 2^-24.
(3) Red zones around every buffer of every entry point under both fills (tests/moat.py): ROWS / FAMILIES, which
    tests/test_xvector_resnet_ragged_host.py holds against the header and the sources; every case also with one broken table entry
    (off + len > T: skipped, nothing written outside, its own columns untouched, the other segments' bits unchanged).
(4) No leak: changing one segment's input leaves every other segment's output bits alone, for the conv and each reduction.
(5) The net: six utterances in one call against `net(wav_i)` (1e-6, the project's bar for batch against single), the norm, the reversed
    batch, the padded form of the argument; the fixture utterances against tests/golden/fx_xvector_resnet.npz (5e-6); a broken utterance;
    the refusals; conv2d_precision = "f16x3".
(6) asv_eval.test_metrics with batch_size 4 against 1 on a toy directory.
The largest error / bound is printed and, if SAT_XVECTOR_RESNET_RAGGED_RATIOS names a file, written there
(profiles/xvector_resnet_ragged_error_ratios.txt).

MEASURED on an MI355X (profiles/xvector_resnet_ragged_error_ratios.txt): every segment kernel has its per-call kernel's bits on every segment |
the conv 0.017 of its float64 bound (the stem 0.48, as the per-call kernels) | the net's rows the SAME BITS as the one-utterance calls, the
reversed batch and the padded form (observed 0; bar 1e-6), 1.8e-7 from the reference's fixtures (bar 5e-6) | test_metrics with batch_size 4:
the same bits as with 1 | a broken utterance: its row all NaN, no other row changes.  The file's 74 tests take 5.5 s on the GPU."""
import functools
import json
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import ref64_resnet
from moat import Buf, run_case
from ref64 import U

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# every SAT_LAUNCH_CHECK string of csrc/ragged2d/ (tests/test_xvector_resnet_ragged_host.py holds this against the sources)
FAMILIES = ["conv2d_segments_mfma_kernel", "conv2d_segments_stem_kernel", "plane_mean_segments_kernel", "se_scale_add_relu_segments_kernel",
            "row_mean_std_segments_kernel"]
WIDTHS = (33, 1, 64, 97, 2, 65, 31, 63, 32)                 # shuffled
WIDTHS_256 = (33, 1, 64)
H_CONV = 5
# (Cin, Cout, ksize, stride)
CONVS = ((1, 32, 3, 1), (32, 32, 3, 1), (32, 64, 3, 2), (32, 64, 1, 2), (64, 64, 3, 1), (64, 128, 3, 2), (128, 256, 1, 2), (256, 256, 3, 1))
EPILOGUES = ("none", "affine", "affine_relu")
REVERSED_CASE = (32, 64, 3, 2, "affine_relu")
PLANES_T = {1: (63, 1, 129, 64, 128, 65), 5: (13, 1, 26, 65, 12, 33), 10: (1, 6, 7, 13, 65, 64)}      # H -> T_i
CHANNELS = (5, 8)
STD_LENGTHS = (65, 2, 129, 63, 3, 64)
NET_SAMPLES = (8000, 10079, 10080, 16000, 24123, 1280)
FIXTURE_UTTERANCES = (("harm0_16000", 0, 16000), ("harm3_48000", 3, 48000), ("harm7_24123", 7, 24123))

_RATIOS = {}


def _note(name, r, what):
    if r > _RATIOS.get(name, (-1.0, ""))[0]:
        _RATIOS[name] = (r, what)


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    lines = [f"{k:56s} {r:10.4f}   at {what}" for k, (r, what) in sorted(_RATIOS.items())]
    print("\nlargest observed error / bound per quantity (0 = the same bits):\n" + "\n".join(lines))
    path = os.environ.get("SAT_XVECTOR_RESNET_RAGGED_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_xvector_resnet_ragged.py: largest observed error / bound per quantity (a ratio above 1 fails; 0 = the same bits)\n")
            f.write("\n".join(lines) + "\n")


def _sat():
    import satools_amd  # noqa: F401
    from satools_amd import _lib, ops
    return _lib, ops


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def out_widths(widths, stride):
    return tuple((w - 1) // stride + 1 for w in widths)


def layout(frames, reverse=False):
    """(off, len, T_tot) as lists; `reverse`: the segments laid out in reverse order (segment B - 1 first), offsets still indexed by i"""
    _, ops = _sat()
    frames = list(frames)
    if reverse:
        off, _, t_tot = ops.ragged_layout(frames[::-1])
        return [int(o) for o in off][::-1], frames, int(t_tot)
    off, length, t_tot = ops.ragged_layout(frames)
    return [int(o) for o in off], [int(n) for n in length], int(t_tot)


def gap_mask(lay, shape):
    """bool [*shape, T_tot]: True on the columns outside every segment"""
    off, length, t_tot = lay
    m = torch.ones(*shape, t_tot, dtype=torch.bool)
    for o, n in zip(off, length):
        m[..., o:o + n] = False
    return m


def pack(segments, lay, fill=float("nan")):
    """per-utterance CPU tensors [..., T_i] -> packed [..., T_tot] with `fill` in the gap columns"""
    off, length, t_tot = lay
    out = torch.full((*segments[0].shape[:-1], t_tot), fill)
    for s, o, n in zip(segments, off, length):
        out[..., o:o + n] = s
    return out


def table(lay):
    _, ops = _sat()
    return ops.RaggedLevel(lay[0], lay[1], lay[2], device=torch.device(DEV))


def _same(name, got, want, what):
    same = torch.equal(got, want)
    _note(name + " (bits)", 0.0 if same else float("inf"), what)
    assert same, (name, what, float((got - want).abs().max()))


def _family(_lib, name):
    assert _lib.lib().sat_last_dispatch_name().decode().split("<")[0].strip() == name


# ---- (1), (2) the conv -----------------------------------------------------------------------------------------------------------
def conv_widths(cin):
    return WIDTHS_256 if cin == 256 else WIDTHS


@functools.lru_cache(maxsize=None)
def conv_case(cin, cout, k, s, epi):
    """per-utterance inputs (CPU, shared, never modified), the float64 value and the derived bound per utterance"""
    g = _gen(31, cin, cout, k, s, len(epi))
    widths = conv_widths(cin)
    xs = tuple(torch.randn(cin, H_CONV, w, generator=g) * (0.5 + 0.25 * i) for i, w in enumerate(widths))
    w = torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5
    sc = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.2, -1.0, 1.0) if "affine" in epi else None
    sh = torch.randn(cout, generator=g) if "affine" in epi else None
    refs = []
    for x in xs:
        want, a = ref64_resnet.conv2d(x.unsqueeze(0), w, s, sc, sh, "relu" in epi)
        kk = 9 * cin + 4
        if sc is None:
            bound = kk * U * a["S"]
        else:
            s64 = sc.double().view(1, -1, 1, 1)
            bound = kk * U * a["S"] * s64.abs() + U * (a["sum"] * s64).abs() + U * a["affine"].abs()
        refs.append((want[0], bound[0]))
    return dict(xs=xs, w=w, sc=sc, sh=sh, relu="relu" in epi, refs=tuple(refs), widths=widths)


def _run_conv(cin, cout, k, s, epi, reverse=False):
    _lib, ops = _sat()
    c = conv_case(cin, cout, k, s, epi)
    lin, lout = layout(c["widths"]), layout(out_widths(c["widths"], s), reverse)
    tin, tout = table(lin), table(lout)
    dev = lambda t: None if t is None else t.to(DEV)
    wp = ops.pack_conv2d_weight(c["w"].to(DEV))
    Ho = (H_CONV - 1) // s + 1
    y = torch.full((1, cout, Ho, tout.T_tot), -7.0, device=DEV)
    got = ops.conv2d_segments(pack(c["xs"], lin).to(DEV).unsqueeze(0), wp, k, s, tin, tout, ch_scale=dev(c["sc"]), ch_shift=dev(c["sh"]), relu=c["relu"], out=y)
    _family(_lib, "conv2d_segments_stem_kernel" if cin == 1 else "conv2d_segments_mfma_kernel")
    assert got.data_ptr() == y.data_ptr()
    tag = f"{cin}->{cout} k{k} s{s} {epi}" + (" reversed output" if reverse else "")
    for i, x in enumerate(c["xs"]):
        what = f"{tag} segment {i} of width {c['widths'][i]}"
        seg = tout.segment(y, i)[0]
        row = ops.conv2d(x.to(DEV).unsqueeze(0), wp, k, s, ch_scale=dev(c["sc"]), ch_shift=dev(c["sh"]), relu=c["relu"])[0]
        _same("conv2d_segments" + (" stem" if cin == 1 else ""), seg, row, what)
        want, bound = c["refs"][i]
        err = (seg.cpu().double() - want).abs()
        ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        r = float(ratio.max())
        _note(f"conv2d_segments k{k} s{s}" + (" stem" if cin == 1 else "") + " vs float64 / derived bound", r, what)
        assert r <= 1.0, (what, r, float(err.max()))
    assert bool((y[0].cpu()[gap_mask(lout, (cout, Ho))] == -7.0).all()), tag


@pytest.mark.gpu
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("cin,cout,k,s", CONVS, ids=lambda v: str(v))
def test_conv2d_segments_has_the_row_kernels_bits_and_the_float64_bound(cin, cout, k, s, epi):
    _run_conv(cin, cout, k, s, epi)


@pytest.mark.gpu
def test_conv2d_segments_output_table_is_independent_of_the_inputs():
    """the output's segments in reverse order: the two tables share nothing but the segment count and the widths"""
    _run_conv(*REVERSED_CASE, reverse=True)


# ---- (1) the reductions and the SE tail -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane_case(C, H, which=0):
    g = _gen(32, C, H, which)
    return tuple(torch.randn(C, H, t, generator=g) * (0.5 + i) + (i - 2.0) for i, t in enumerate(PLANES_T[H]))


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("H", sorted(PLANES_T))
def test_plane_mean_segments_is_the_row_kernel_on_the_utterances_own_plane(C, H):
    _, ops = _sat()
    xs, lay = plane_case(C, H), layout(PLANES_T[H])
    m = ops.plane_mean_segments(pack(xs, lay).to(DEV).unsqueeze(0), table(lay))
    assert m.shape == (len(xs), C)
    for i, x in enumerate(xs):
        _same("plane_mean_segments", m[i], ops.row_mean(x.reshape(1, C, -1).to(DEV))[0, :, 0], f"C {C} H {H} segment {i} of {PLANES_T[H][i]} ({H * PLANES_T[H][i]} elements)")


@functools.lru_cache(maxsize=None)
def std_case(R, which=0):
    g = _gen(33, R, which)
    return tuple(torch.randn(R, t, generator=g) * (0.5 + i) + (i - 2.0) for i, t in enumerate(STD_LENGTHS))


@pytest.mark.gpu
@pytest.mark.parametrize("R", CHANNELS)
def test_row_mean_std_segments_is_the_row_kernel_per_segment(R):
    _, ops = _sat()
    xs, lay = std_case(R), layout(STD_LENGTHS)
    out = ops.row_mean_std_segments(pack(xs, lay).to(DEV).unsqueeze(0), table(lay))
    assert out.shape == (len(xs), 2 * R)
    for i, x in enumerate(xs):
        _same("row_mean_std_segments", out[i], ops.row_mean_std(x.to(DEV).unsqueeze(0))[0], f"R {R} segment {i} of {STD_LENGTHS[i]}")


@functools.lru_cache(maxsize=None)
def tail_case(C, which):
    g = _gen(34, C, which)
    return tuple(torch.randn(C, H_CONV, w, generator=g) for w in WIDTHS)


def tail_gates(C):
    return torch.randn(len(WIDTHS), C, generator=_gen(35, C)) * 3


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_se_scale_add_relu_segments_is_the_row_kernel_per_segment(C):
    _, ops = _sat()
    zs, rs, g, lay = tail_case(C, 0), tail_case(C, 1), tail_gates(C).to(DEV), layout(WIDTHS)
    y = torch.full((1, C, H_CONV, lay[2]), -7.0, device=DEV)
    tab = table(lay)
    ops.se_scale_add_relu_segments(pack(zs, lay).to(DEV).unsqueeze(0), g, pack(rs, lay).to(DEV).unsqueeze(0), tab, out=y)
    for i in range(len(WIDTHS)):
        want = ops.se_scale_add_relu(zs[i].to(DEV).unsqueeze(0), g[i:i + 1], rs[i].to(DEV).unsqueeze(0))[0]
        _same("se_scale_add_relu_segments", tab.segment(y, i)[0], want, f"C {C} segment {i} of width {WIDTHS[i]}")
    assert bool((y[0].cpu()[gap_mask(lay, (C, H_CONV))] == -7.0).all())


# ---- (3) red zones (tests/moat.py) -----------------------------------------------------------------------------------------------
@dataclass
class Row:
    entry: str                   # the C-ABI function
    name: str
    shapes: list
    make: object                 # make(*shape) -> (specs, call, ref)  (runs on the GPU box only)


ROWS = []
BROKEN = 3                       # the segment whose table entry the `broken` cases spoil


def _ibuf(name, values):
    t = torch.tensor([int(v) for v in values], dtype=torch.int32)
    return Buf(name, "in", t.shape, torch.int32, data=t, index=True)


def _spoil(lay, broken):
    """the table with segment BROKEN running one column past T_tot (off + len > T_tot), or the table itself"""
    off, length, t_tot = lay
    length = list(length)
    if broken:
        length[BROKEN] = t_tot - off[BROKEN] + 1
    return length


def _skipped(lay, shape):
    """bool [*shape, T_tot]: the columns the spoiled entry names inside the buffer (they stay unwritten)"""
    m = torch.zeros(*shape, lay[2], dtype=torch.bool)
    m[..., lay[0][BROKEN]:lay[0][BROKEN] + lay[1][BROKEN]] = True
    return m


def _conv_bounds(cin, cout, k, s, epi, broken):
    """broken: "" | "in" (the input entry runs past T_in) | "out" (the output offset leaves no room for the segment's columns)"""
    _lib, ops = _sat()
    c = conv_case(cin, cout, k, s, epi)
    widths = c["widths"]
    lin, lout = layout(widths), layout(out_widths(widths, s))
    B, Ho, T_in, T_out = len(widths), (H_CONV - 1) // s + 1, lin[2], lout[2]
    out_off = list(lout[0])
    if broken == "out":
        out_off[BROKEN] = T_out - lout[1][BROKEN] + 1
    untouched = gap_mask(lout, (cout, Ho))
    if broken:
        untouched |= _skipped(lout, (cout, Ho))
    wp = c["w"].permute(2, 3, 1, 0).reshape(k * k, cin, cout).contiguous()          # ops.pack_conv2d_weight
    specs = [_ibuf("in_off", lin[0]), _ibuf("in_len", _spoil(lin, broken == "in")), _ibuf("out_off", out_off),
             Buf("x", "in", (cin, H_CONV, T_in), data=pack(c["xs"], lin, 0.0), dontcare=gap_mask(lin, (cin, H_CONV))),
             Buf("y", "out", (cout, Ho, T_out), untouched=untouched), Buf("w", "in", wp.shape, data=wp)]
    if c["sc"] is not None:
        specs += [Buf("scale", "in", (cout,), data=c["sc"]), Buf("shift", "in", (cout,), data=c["sh"])]

    def call(t):
        P = lambda n: t[n].data_ptr() if n in t else None
        _lib.check(_lib.lib().sat_conv2d_segments_f32(P("x"), P("w"), P("y"), P("scale"), P("shift"), int(c["relu"]), P("in_off"), P("in_len"), P("out_off"), B,
                                                      max(widths), cin, cout, H_CONV, T_in, T_out, k, s, _lib.stream()), "conv2d_segments")
        _family(_lib, "conv2d_segments_stem_kernel" if cin == 1 else "conv2d_segments_mfma_kernel")

    def ref(t):
        dev = lambda v: None if v is None else v.to(DEV)
        for i, x in enumerate(c["xs"]):
            if broken and i == BROKEN:
                continue
            want = ops.conv2d(x.to(DEV).unsqueeze(0), wp.to(DEV), k, s, ch_scale=dev(c["sc"]), ch_shift=dev(c["sh"]), relu=c["relu"])[0]
            assert torch.equal(t["y"][..., lout[0][i]:lout[0][i] + lout[1][i]], want), i
    return specs, call, ref


def _plane_bounds(C, H, broken):
    _lib, ops = _sat()
    xs, lay = plane_case(C, H), layout(PLANES_T[H])
    B, T = len(xs), lay[2]
    skipped = torch.zeros(B, C, dtype=torch.bool)
    skipped[BROKEN] = bool(broken)
    specs = [_ibuf("seg_off", lay[0]), _ibuf("seg_len", _spoil(lay, broken)), Buf("x", "in", (C, H, T), data=pack(xs, lay, 0.0), dontcare=gap_mask(lay, (C, H))),
             Buf("y", "out", (B, C), untouched=skipped)]

    def call(t):
        P = lambda n: t[n].data_ptr()
        _lib.check(_lib.lib().sat_plane_mean_segments_f32(P("x"), P("y"), P("seg_off"), P("seg_len"), C, H, B, T, _lib.stream()), "plane_mean_segments")
        _family(_lib, "plane_mean_segments_kernel")

    def ref(t):
        for i, x in enumerate(xs):
            if not (broken and i == BROKEN):
                assert torch.equal(t["y"][i], ops.row_mean(x.reshape(1, C, -1).to(DEV))[0, :, 0]), i
    return specs, call, ref


def _std_bounds(R, broken):
    _lib, ops = _sat()
    xs, lay = std_case(R), layout(STD_LENGTHS)
    B, T = len(xs), lay[2]
    skipped = torch.zeros(B, 2 * R, dtype=torch.bool)
    skipped[BROKEN] = bool(broken)
    specs = [_ibuf("seg_off", lay[0]), _ibuf("seg_len", _spoil(lay, broken)), Buf("x", "in", (R, T), data=pack(xs, lay, 0.0), dontcare=gap_mask(lay, (R,))),
             Buf("out", "out", (B, 2 * R), untouched=skipped)]

    def call(t):
        P = lambda n: t[n].data_ptr()
        _lib.check(_lib.lib().sat_row_mean_std_segments_f32(P("x"), P("out"), P("seg_off"), P("seg_len"), R, B, T, _lib.stream()), "row_mean_std_segments")
        _family(_lib, "row_mean_std_segments_kernel")

    def ref(t):
        for i, x in enumerate(xs):
            if not (broken and i == BROKEN):
                assert torch.equal(t["out"][i], ops.row_mean_std(x.to(DEV).unsqueeze(0))[0]), i
    return specs, call, ref


def _tail_bounds(C, broken):
    _lib, ops = _sat()
    zs, rs, g, lay = tail_case(C, 0), tail_case(C, 1), tail_gates(C), layout(WIDTHS)
    B, T = len(WIDTHS), lay[2]
    gap = gap_mask(lay, (C, H_CONV))
    untouched = gap | _skipped(lay, (C, H_CONV)) if broken else gap
    specs = [_ibuf("seg_off", lay[0]), _ibuf("seg_len", _spoil(lay, broken)), Buf("z", "in", (C, H_CONV, T), data=pack(zs, lay, 0.0), dontcare=gap),
             Buf("r", "in", (C, H_CONV, T), data=pack(rs, lay, 0.0), dontcare=gap), Buf("g", "in", (B, C), data=g), Buf("y", "out", (C, H_CONV, T), untouched=untouched)]

    def call(t):
        P = lambda n: t[n].data_ptr()
        _lib.check(_lib.lib().sat_se_scale_add_relu_segments_f32(P("z"), P("g"), P("r"), P("y"), P("seg_off"), P("seg_len"), B, max(WIDTHS), C, H_CONV, T,
                                                                 _lib.stream()), "se_scale_add_relu_segments")
        _family(_lib, "se_scale_add_relu_segments_kernel")

    def ref(t):
        for i in range(B):
            if not (broken and i == BROKEN):
                want = ops.se_scale_add_relu(zs[i].to(DEV).unsqueeze(0), g[i:i + 1].to(DEV), rs[i].to(DEV).unsqueeze(0))[0]
                assert torch.equal(t["y"][..., lay[0][i]:lay[0][i] + lay[1][i]], want), i
    return specs, call, ref


ROWS.append(Row("sat_conv2d_segments_f32", "conv", [(1, 32, 3, 1, "affine_relu", b) for b in ("", "in", "out")] + [(32, 32, 3, 1, "none", b) for b in ("", "in")]
                + [(32, 64, 3, 2, "affine_relu", b) for b in ("", "in", "out")] + [(128, 256, 1, 2, "affine", b) for b in ("", "in")], _conv_bounds))
ROWS.append(Row("sat_plane_mean_segments_f32", "plane mean", [(C, H, b) for C in CHANNELS for H in (1, 5) for b in (False, True)], _plane_bounds))
ROWS.append(Row("sat_row_mean_std_segments_f32", "mean std", [(R, b) for R in CHANNELS for b in (False, True)], _std_bounds))
ROWS.append(Row("sat_se_scale_add_relu_segments_f32", "tail", [(C, b) for C in CHANNELS for b in (False, True)], _tail_bounds))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [(r, s) for r in ROWS for s in r.shapes], ids=lambda p: f"{p[0].entry[4:]}:{p[0].name}-" + "x".join(str(v) for v in p[1]))
def test_no_access_outside_the_buffers(p):
    r, shape = p
    specs, call, ref = r.make(*shape)
    v, m, plain = run_case(specs, call, DEV, sync=torch.cuda.synchronize)
    assert not v, f"{r.entry} [{r.name}] {shape}:\n" + "\n".join(str(x) for x in v)
    ref(m.t)


# ---- (4) no leak between segments ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_changing_one_segment_leaves_every_other_segments_bits_alone(fill):
    _, ops = _sat()
    j = 4
    # the conv (a stride-2 3x3: every segment's halo reaches into the gap and, without the select, into its neighbours)
    cin, cout, k, s, epi = REVERSED_CASE
    c = conv_case(cin, cout, k, s, epi)
    lin, lout = layout(c["widths"]), layout(out_widths(c["widths"], s))
    tin, tout = table(lin), table(lout)
    wp = ops.pack_conv2d_weight(c["w"].to(DEV))
    dirty = lambda segs: tuple(torch.full_like(x, fill) if i == j else x for i, x in enumerate(segs))
    run = lambda xs: ops.conv2d_segments(pack(xs, lin, fill).to(DEV).unsqueeze(0), wp, k, s, tin, tout, ch_scale=c["sc"].to(DEV), ch_shift=c["sh"].to(DEV), relu=True)
    a, b = run(c["xs"]), run(dirty(c["xs"]))
    for i in range(len(c["widths"])):
        if i != j:
            assert torch.equal(tout.segment(a, i), tout.segment(b, i)), ("conv", i)
    C = 5
    lay = layout(PLANES_T[5])
    a, b = (ops.plane_mean_segments(pack(xs, lay, fill).to(DEV).unsqueeze(0), table(lay)) for xs in (plane_case(C, 5), dirty(plane_case(C, 5))))
    keep = [i for i in range(a.shape[0]) if i != j]
    assert torch.equal(a[keep], b[keep]) and bool(torch.isfinite(a).all())
    lay = layout(STD_LENGTHS)
    a, b = (ops.row_mean_std_segments(pack(xs, lay, fill).to(DEV).unsqueeze(0), table(lay)) for xs in (std_case(C), dirty(std_case(C))))
    assert torch.equal(a[keep], b[keep]) and bool(torch.isfinite(a).all())
    lay, g = layout(WIDTHS), tail_gates(C).to(DEV)
    tab = table(lay)
    a, b = (ops.se_scale_add_relu_segments(pack(zs, lay, fill).to(DEV).unsqueeze(0), g, pack(tail_case(C, 1), lay, fill).to(DEV).unsqueeze(0), tab,
                                           out=torch.zeros(1, C, H_CONV, lay[2], device=DEV)) for zs in (tail_case(C, 0), dirty(tail_case(C, 0))))
    for i in range(len(WIDTHS)):
        if i != j:
            assert torch.equal(tab.segment(a, i), tab.segment(b, i)), ("tail", i)


# ---- (5) the net -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    import satools_amd  # noqa: F401
    from satools_amd import synthetic, xvector_resnet
    m = xvector_resnet.build()(num_speakers=10)
    m.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def net_wavs():
    from satools_amd import synthetic
    return tuple(synthetic.harm_batch([10 + i], n)[0] for i, n in enumerate(NET_SAMPLES))


@pytest.fixture(scope="module")
def clean_rows(net):
    return net.extract_batch([w.to(DEV) for w in net_wavs()])


@pytest.mark.gpu
def test_ragged_batch_matches_the_single_calls_its_reversed_order_and_the_padded_form(net, clean_rows):
    wavs = net_wavs()
    assert clean_rows.shape == (len(wavs), 256) and net.last_conv2d_arithmetic == "f32"
    back = net.extract_batch([w.to(DEV) for w in reversed(wavs)])
    padded = torch.full((len(wavs), max(NET_SAMPLES) + 7), float("nan"))
    for i, w in enumerate(wavs):
        padded[i, :w.shape[0]] = w
    assert torch.equal(net.extract_batch((padded.to(DEV), list(NET_SAMPLES))), clean_rows)           # the padded form of the argument, NaN past each end
    assert torch.equal(net.extract_batch((padded.to(DEV), torch.tensor(NET_SAMPLES))), clean_rows)
    for i, w in enumerate(wavs):
        what = f"utterance {i} of {NET_SAMPLES[i]} samples"
        one = float((clean_rows[i] - net(w.to(DEV))[1][0]).abs().max())
        rev = float((clean_rows[i] - back[len(wavs) - 1 - i]).abs().max())
        nrm = abs(float(clean_rows[i].cpu().double().norm()) - 1.0)
        print(f"{what}: vs the one-utterance call {one:.2e}, vs the reversed batch {rev:.2e}, | norm - 1 | {nrm:.2e}")
        _note("net row vs one-utterance call / 1e-6", one / 1e-6, what)
        _note("net row vs reversed order / 1e-6", rev / 1e-6, what)
        _note("net | norm - 1 | / 1e-5", nrm / 1e-5, what)
        assert one < 1e-6 and rev < 1e-6 and nrm < 1e-5, what


@pytest.mark.gpu
def test_the_fixture_utterances_in_one_ragged_call_match_the_reference(net):
    from satools_amd import synthetic
    fx = np.load(os.path.join(GOLD, "fx_xvector_resnet.npz"))
    rows = net.extract_batch([synthetic.harm_batch([seed], n)[0].to(DEV) for _, seed, n in FIXTURE_UTTERANCES])
    for i, (tag, _, _) in enumerate(FIXTURE_UTTERANCES):
        got, ref = rows[i].cpu().numpy(), fx[tag + "/xvector"][0]
        err, cos = float(np.abs(got - ref).max()), float((got.astype(np.float64) * ref).sum())
        print(f"{tag}: ragged row max abs error vs reference {err:.2e}, cosine {cos:.7f}")
        _note("net row vs reference fixture / 5e-6", err / 5e-6, tag)
        assert err < 5e-6 and cos > 0.999999 and abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [2, 1])
@pytest.mark.parametrize("how", ["all NaN", "one NaN sample", "one infinite sample"])
def test_a_broken_utterance_gives_a_nan_row_and_changes_no_other_rows_bits(net, bad, how):
    """layout and dispatch are identical in the two calls and no output column may depend on another segment or on a gap: every other row
    keeps its bits.  The broken utterance's own row is NaN: its whole feature segment is (the InstanceNorm's mean), and extract_batch
    carries that past the ReLUs of the conv epilogues, which are max(v, 0) and give 0 for NaN (`forward` returns a finite vector there)"""
    wavs = [net_wavs()[i].to(DEV) for i in (1, 3, 5)]                             # 10079, 16000 and 1280 samples
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


@pytest.mark.gpu
def test_extract_batch_refusals(net):
    from satools_amd._lib import SatError
    ok = net_wavs()[0].to(DEV)
    with pytest.raises(SatError, match=r"utterance 1 of 1279 samples"):
        net.extract_batch([ok, ok[:1279], ok])
    with pytest.raises(SatError, match=r"utterance 2 of 1279 samples"):
        net.extract_batch((torch.zeros(3, 8000, device=DEV), [8000, 1280, 1279]))
    with pytest.raises(SatError, match="1025 utterances"):
        net.extract_batch([ok[:1300]] * 1025)
    with pytest.raises(SatError, match="no CPU fallback"):
        net.extract_batch([ok, ok.cpu()])
    with pytest.raises(SatError, match="empty"):
        net.extract_batch([])
    with pytest.raises(SatError, match="1-D"):
        net.extract_batch([ok.unsqueeze(0)])
    with pytest.raises(SatError, match="lengths"):
        net.extract_batch((torch.zeros(2, 8000, device=DEV), [8000, 9000]))
    # [32][80][T_tot_0] of 2^31 bytes: 209 716 frames; the rows are views of one short buffer (nothing that large is allocated)
    long = torch.zeros(160 * 2100, device=DEV)
    with pytest.raises(SatError, match="2\\^31 bytes"):
        net.extract_batch([long] * 100)
    assert net.extract_batch([ok]).shape == (1, 256)                              # no sticky error


@pytest.mark.gpu
def test_extract_batch_runs_the_convs_in_f32_whatever_conv2d_precision_says(net, clean_rows):
    wavs = [w.to(DEV) for w in net_wavs()]
    try:
        net.conv2d_precision = "f16x3"                                            # an instance attribute over the class's default
        net(wavs[0])
        assert net.last_conv2d_arithmetic == "f16x3"
        rows = net.extract_batch(wavs)
        assert net.last_conv2d_arithmetic == "f32"
    finally:
        del net.conv2d_precision
    assert torch.equal(rows, clean_rows)


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
    model = satools_amd.load_model("synthetic:xvector_resnet?speakers=12").to(DEV)
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
    assert ma == mb
    assert [l.split()[:2] for l in open(tmp_path / "one" / "scores")] == [l.split()[:2] for l in open(tmp_path / "four" / "scores")]
