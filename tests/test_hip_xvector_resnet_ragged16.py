"""Split-f16 2-D convs in the ragged batches of the ResNet x-vector extractor (csrc/ragged2d16/, include/satools_hip_ragged2d16.h;
xvector_resnet.Net.ragged_conv2d_precision = "f16x3") on the HIP device.  Needs a real MI355X: run with `-m gpu`.
Every input has NaN in its gap columns unless a test says otherwise.

(a) Bits: every segment of sat_conv2d_f16x3_segments_f32's result torch.equal to ops.conv2d_f16x3 on that utterance alone.  H = 5 (two row
    tiles, one row in the second; Ho = 3 at stride 2), widths 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129 in a shuffled order (around the
    64-column tile at stride 1, around the 32-column tile at stride 2 through Wo = 32 / 32 / 33), one (Cin -> Cout, k, s) per instantiation
    of the kernel plus 256 -> 256 on three widths (16 chunks of K), under the epilogues none / affine / affine + ReLU, and one case whose
    output table has the segments in reverse order.
(b) The same cases against tests/ref64_resnet.conv2d per utterance, under the per-call kernel's derived bound (tests/test_hip_conv2d16.py):
        |err| <= ((27 Cin + 4) U + 2^-21) sum|w x| |scale|  +  2^-24 sum|w| |scale|  +  U |sum scale|  +  U |sum scale + shift|,  U = 2^-24.
(c) Flags: 65520.0, +inf and NaN inside segment i of three raise flag i alone and leave the other segments' bits; the largest f32 below
    65520 raises nothing; gaps of NaN / inf / 1e30 raise nothing; a flag preset to 1 stays 1.
(d) Red zones around every buffer of the entry point, the flags included, under both fills (tests/moat.py): ROWS / FAMILIES, which
    tests/test_xvector_resnet_ragged16_host.py holds against the header and the sources; every shape also with one broken table entry
    (off + len > T: skipped, nothing written outside, its own columns and flag untouched, the other segments' bits unchanged).
(e) No leak: changing one segment's input leaves every other segment's output bits alone.
(f) The net: the ragged f16x3 rows of NET_SAMPLES against net16(wav_i) (conv2d_precision = "f16x3") at 1e-6, the reversed batch, the padded
    form of the argument, the fixture utterances against tests/golden/fx_xvector_resnet.npz (5e-6), the bookkeeping, a NaN utterance.
(g) Fallback: every row (one block's BatchNorm scale raised) and one row of four (a click in silence beside short harmonic utterances under
    the stem scale PARTIAL_STEM_SCALE, which tests/test_xvector_resnet_ragged16_host.py holds against the float64 forward on the CPU).
(h) ragged_conv2d_precision left at "f32": extract_batch's rows bit for bit, whatever conv2d_precision says.
The largest error / bound is printed and, if SAT_XVECTOR_RESNET_RAGGED16_RATIOS names a file, written there
(profiles/xvector_resnet_ragged16_error_ratios.txt).

MEASURED on an MI355X (profiles/xvector_resnet_ragged16_error_ratios.txt): every segment has the per-call kernel's bits | largest error /
float64 bound 0.0036 (3x3 stride 1), 0.0032 (3x3 stride 2), 0.0055 (1x1 stride 1), 0.0061 (1x1 stride 2): the per-call kernel's figures |
the net's ragged f16x3 rows the SAME BITS as the one-utterance f16x3 calls, the reversed batch and the padded form (observed 0; bar 1e-6),
2.1e-7 from the reference's fixtures (bar 5e-6) | both fallbacks as described.  The file's 53 tests take 4.1 s on the GPU."""
import functools
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import ref64_resnet
from moat import Buf, run_case
from ref64 import U
from test_hip_xvector_resnet_ragged import _family, _gen, _ibuf, _sat, gap_mask, layout, out_widths, pack, table

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRY = "sat_conv2d_f16x3_segments_f32"
FAMILIES = ["conv2d_segments_f16x3_kernel"]   # every SAT_LAUNCH_CHECK string of csrc/ragged2d16/ (the host test holds this against the sources)
TH, TW1, TW2 = 4, 64, 32                      # csrc/ragged2d16/: output rows per block; output columns per block at stride 1 / 2
WIDTHS = (33, 1, 128, 64, 129, 2, 65, 31, 127, 63, 32)      # shuffled
WIDTHS_256 = (33, 1, 128)
H_CONV = 5
# (Cin, Cout, ksize, stride): one per instantiation <3,1,1,2> <3,1,2,2> <3,2,1,1> <1,2,1,1> <1,1,1,2> <1,1,2,2>, a second 1x1 stride 2, 16 chunks of K
CONVS = ((32, 32, 3, 1), (64, 64, 3, 1), (32, 64, 3, 2), (32, 64, 1, 2), (32, 32, 1, 1), (32, 64, 1, 1), (128, 256, 1, 2), (256, 256, 3, 1))
EPILOGUES = ("none", "affine", "affine_relu")
REVERSED_CASE = (32, 64, 3, 2, "affine_relu")
FLAG_CASE = (64, 64, 3, 1, "affine")          # on its first three widths
SPLIT_LIMIT = 65520.0                         # SAT_CONV2D16_SPLIT_LIMIT
NET_SAMPLES = (8000, 10079, 10080, 16000, 24123, 1280)
FIXTURE_UTTERANCES = (("harm0_16000", 0, 16000), ("harm3_48000", 3, 48000), ("harm7_24123", 7, 24123))
ALL_FALLBACK_KEY, ALL_FALLBACK_FACTOR = "sequence_network.layer1.0.bn1.weight", 1e6
# (g) partial fallback: utterance PARTIAL_CLICK is one click in 30 s of silence (its InstanceNorm'd features peak near sqrt(frames)), the
# others are short harmonic utterances (seed, samples); the stem's BatchNorm weight times PARTIAL_STEM_SCALE puts the click's largest conv
# input above 4 x 65520 and every other utterance's below 65520 / 4 in the float64 forward (asserted on the CPU by the host test)
PARTIAL_HARMONIC = ((20, 1280), (23, 1440), (21, 1600))
PARTIAL_CLICK, PARTIAL_CLICK_SAMPLES = 1, 480000
PARTIAL_STEM_SCALE = 850.0

_RATIOS = {}


def _note(name, r, what):
    if r > _RATIOS.get(name, (-1.0, ""))[0]:
        _RATIOS[name] = (r, what)


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    lines = [f"{k:60s} {r:10.4f}   at {what}" for k, (r, what) in sorted(_RATIOS.items())]
    print("\nlargest observed error / bound per quantity (0 = the same bits):\n" + "\n".join(lines))
    path = os.environ.get("SAT_XVECTOR_RESNET_RAGGED16_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_xvector_resnet_ragged16.py: largest observed error / bound per quantity (a ratio above 1 fails; 0 = the same bits)\n")
            f.write("\n".join(lines) + "\n")


def _same(name, got, want, what):
    same = torch.equal(got, want)
    _note(name + " (bits)", 0.0 if same else float("inf"), what)
    assert same, (name, what, float((got - want).abs().max()))


# ---- (a), (b) the conv ---------------------------------------------------------------------------------------------------------------
def conv_widths(cin):
    return WIDTHS_256 if cin == 256 else WIDTHS


@functools.lru_cache(maxsize=None)
def conv_case(cin, cout, k, s, epi):
    """per-utterance inputs (CPU, shared, never modified), the float64 value and the per-call kernel's derived bound per utterance"""
    g = _gen(36, cin, cout, k, s, len(epi))
    widths = conv_widths(cin)
    xs = tuple(torch.randn(cin, H_CONV, w, generator=g) * (0.5 + 0.25 * i) for i, w in enumerate(widths))
    w = torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5
    sc = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.2, -1.0, 1.0) if "affine" in epi else None
    sh = torch.randn(cout, generator=g) if "affine" in epi else None
    kk = (27 * cin + 4) * U + 2.0 ** -21
    wsum = w.double().abs().sum((1, 2, 3)).view(1, -1, 1, 1)
    refs = []
    for x in xs:
        want, a = ref64_resnet.conv2d(x.unsqueeze(0), w, s, sc, sh, "relu" in epi)
        if sc is None:
            bound = kk * a["S"] + 2.0 ** -24 * wsum
        else:
            s64 = sc.double().view(1, -1, 1, 1)
            bound = kk * a["S"] * s64.abs() + 2.0 ** -24 * wsum * s64.abs() + U * (a["sum"] * s64).abs() + U * a["affine"].abs()
        refs.append((want[0], bound[0]))
    return dict(xs=xs, w=w, sc=sc, sh=sh, relu="relu" in epi, refs=tuple(refs), widths=widths)


def _dev(t):
    return None if t is None else t.to(DEV)


_SPLIT = {}


def _split(c):
    """the case's split weights on the device, packed once (the cases live as long as the module)"""
    _, ops = _sat()
    if id(c["w"]) not in _SPLIT:
        _SPLIT[id(c["w"])] = ops.pack_conv2d_weight_f16x3(c["w"].to(DEV))
    return _SPLIT[id(c["w"])]


def _segments(c, k, s, xs, lin, tin, tout, flags=None, out=None, fill=float("nan")):
    _, ops = _sat()
    w16, d = _split(c)
    return ops.conv2d_f16x3_segments(pack(xs, lin, fill).to(DEV).unsqueeze(0), w16, d, k, s, tin, tout, ch_scale=_dev(c["sc"]), ch_shift=_dev(c["sh"]),
                                     relu=c["relu"], overflow=flags, out=out)


def _alone(c, k, s, x, flag=None):
    _, ops = _sat()
    w16, d = _split(c)
    return ops.conv2d_f16x3(x.to(DEV).unsqueeze(0), w16, d, k, s, ch_scale=_dev(c["sc"]), ch_shift=_dev(c["sh"]), relu=c["relu"], overflow=flag)[0]


def _run_conv(cin, cout, k, s, epi, reverse=False):
    _lib, ops = _sat()
    c = conv_case(cin, cout, k, s, epi)
    lin, lout = layout(c["widths"]), layout(out_widths(c["widths"], s), reverse)
    tin, tout = table(lin), table(lout)
    Ho = (H_CONV - 1) // s + 1
    y = torch.full((1, cout, Ho, tout.T_tot), -7.0, device=DEV)
    flags = torch.zeros(len(c["widths"]), dtype=torch.int32, device=DEV)
    got = _segments(c, k, s, c["xs"], lin, tin, tout, flags, y)
    _family(_lib, FAMILIES[0])
    assert got.data_ptr() == y.data_ptr()
    tag = f"{cin}->{cout} k{k} s{s} {epi}" + (" reversed output" if reverse else "")
    for i, x in enumerate(c["xs"]):
        what = f"{tag} segment {i} of width {c['widths'][i]}"
        seg = tout.segment(y, i)[0]
        _same("conv2d_f16x3_segments", seg, _alone(c, k, s, x), what)                 # (a)
        want, bound = c["refs"][i]                                                  # (b)
        err = (seg.cpu().double() - want).abs()
        ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        r = float(ratio.max())
        print(f"{what}: error / bound {r:.4f}")
        _note(f"conv2d_f16x3_segments k{k} s{s} vs float64 / derived bound", r, what)
        assert r <= 1.0, (what, r, float(err.max()))
    assert bool((y[0].cpu()[gap_mask(lout, (cout, Ho))] == -7.0).all()), tag          # only segment columns are written
    assert not bool(flags.any()), tag                                               # NaN gaps raise no flag


@pytest.mark.gpu
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("cin,cout,k,s", CONVS, ids=lambda v: str(v))
def test_conv2d_f16x3_segments_has_the_per_call_kernels_bits_and_the_float64_bound(cin, cout, k, s, epi):
    _run_conv(cin, cout, k, s, epi)


@pytest.mark.gpu
def test_conv2d_f16x3_segments_output_table_is_independent_of_the_inputs():
    """the output's segments in reverse order: the two tables share nothing but the segment count and the widths"""
    _run_conv(*REVERSED_CASE, reverse=True)


# ---- (c) flags -----------------------------------------------------------------------------------------------------------------------
def _flag_setup():
    cin, cout, k, s, epi = FLAG_CASE
    c = conv_case(cin, cout, k, s, epi)
    xs = c["xs"][:3]
    lay = layout(c["widths"][:3])
    return c, k, s, xs, lay, table(lay)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [SPLIT_LIMIT, float("inf"), float("nan")], ids=str)
def test_a_value_outside_the_range_raises_its_own_segments_flag_alone(value):
    c, k, s, xs, lay, tab = _flag_setup()
    clean = _segments(c, k, s, xs, lay, tab, tab)
    for i in range(3):
        dirty = list(xs)
        dirty[i] = xs[i].clone()
        dirty[i][37, 2, xs[i].shape[-1] // 2] = value
        flags = torch.zeros(3, dtype=torch.int32, device=DEV)
        y = _segments(c, k, s, dirty, lay, tab, tab, flags)
        got = flags.tolist()
        assert got[i] != 0 and [f for j, f in enumerate(got) if j != i] == [0, 0], (value, i, got)
        for j in range(3):
            if j != i:
                assert torch.equal(tab.segment(y, j), tab.segment(clean, j)), (value, i, j)
        _segments(c, k, s, dirty, lay, tab, tab, None)                             # a null pointer: don't report
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_the_largest_splittable_value_and_the_gaps_raise_nothing_and_a_raised_flag_stays():
    c, k, s, xs, lay, tab = _flag_setup()
    edge = [x.clone() for x in xs]
    for x in edge:
        x[5, 0, 0] = float(np.nextafter(np.float32(SPLIT_LIMIT), np.float32(0.0)))
        x[11, 4, -1] = -float(np.nextafter(np.float32(SPLIT_LIMIT), np.float32(0.0)))
    flags = torch.zeros(3, dtype=torch.int32, device=DEV)
    _segments(c, k, s, edge, lay, tab, tab, flags)
    assert flags.tolist() == [0, 0, 0]
    clean = _segments(c, k, s, xs, lay, tab, tab)
    for fill in (float("nan"), float("inf"), -float("inf"), 1e30):
        y = _segments(c, k, s, xs, lay, tab, tab, flags, fill=fill)
        assert flags.tolist() == [0, 0, 0], fill
        for i in range(3):
            assert torch.equal(tab.segment(y, i), tab.segment(clean, i)), (fill, i)   # nor do they reach a result
    flags.copy_(torch.tensor([0, 1, 0], dtype=torch.int32))
    _segments(c, k, s, xs, lay, tab, tab, flags)                                   # a clean call leaves a raised flag raised, and raises no other
    assert flags.tolist() == [0, 1, 0]


# ---- (d) red zones (tests/moat.py) -------------------------------------------------------------------------------------------------
@dataclass
class Row:
    entry: str                   # the C-ABI function
    name: str
    shapes: list
    make: object                 # make(*shape) -> (specs, call, ref)  (runs on the GPU box only)


ROWS = []
BROKEN = 3                       # the segment whose table entry the `broken` cases spoil


def _conv_bounds(cin, cout, k, s, epi, broken):
    """broken: "" | "in" (the input entry runs past T_in) | "out" (the output offset leaves no room for the segment's columns)"""
    _lib, ops = _sat()
    c = conv_case(cin, cout, k, s, epi)
    widths, xs = c["widths"], c["xs"]
    lin, lout = layout(widths), layout(out_widths(widths, s))
    B, Ho, T_in, T_out = len(widths), (H_CONV - 1) // s + 1, lin[2], lout[2]
    in_len, out_off = list(lin[1]), list(lout[0])
    if broken == "in":
        in_len[BROKEN] = T_in - lin[0][BROKEN] + 1
    if broken == "out":
        out_off[BROKEN] = T_out - lout[1][BROKEN] + 1
    untouched = gap_mask(lout, (cout, Ho))
    if broken:
        untouched[..., lout[0][BROKEN]:lout[0][BROKEN] + lout[1][BROKEN]] = True
    w16, d = _split(c)
    w16 = w16.cpu()
    specs = [_ibuf("in_off", lin[0]), _ibuf("in_len", in_len), _ibuf("out_off", out_off),
             Buf("x", "in", (cin, H_CONV, T_in), data=pack(xs, lin, 0.0), dontcare=gap_mask(lin, (cin, H_CONV))),
             Buf("y", "out", (cout, Ho, T_out), untouched=untouched), Buf("w_split", "in", w16.shape, torch.float16, data=w16),
             Buf("flags", "inout", (B,), torch.int32, data=torch.zeros(B, dtype=torch.int32))]
    if c["sc"] is not None:
        specs += [Buf("scale", "in", (cout,), data=c["sc"]), Buf("shift", "in", (cout,), data=c["sh"])]

    def call(t):
        P = lambda n: t[n].data_ptr() if n in t else None
        _lib.check(_lib.lib().sat_conv2d_f16x3_segments_f32(P("x"), P("w_split"), d, P("y"), P("scale"), P("shift"), int(c["relu"]), P("in_off"), P("in_len"),
                                                            P("out_off"), B, max(widths), cin, cout, H_CONV, T_in, T_out, k, s, P("flags"), _lib.stream()), ENTRY)
        _family(_lib, FAMILIES[0])

    def ref(t):
        for i, x in enumerate(xs):
            if broken and i == BROKEN:
                continue
            assert torch.equal(t["y"][..., lout[0][i]:lout[0][i] + lout[1][i]], _alone(c, k, s, x)), i
        assert t["flags"].tolist() == [0] * B                                      # the fills of the gaps (NaN, 5.1e4) and the zones raise nothing
    return specs, call, ref


ROWS.append(Row(ENTRY, "conv", [(32, 32, 3, 1, "none", b) for b in ("", "in", "out")] + [(64, 64, 3, 1, "affine_relu", b) for b in ("", "in")]
                + [(32, 64, 3, 2, "affine_relu", b) for b in ("", "in", "out")] + [(32, 64, 1, 2, "affine", b) for b in ("", "out")]
                + [(32, 32, 1, 1, "none", b) for b in ("", "in")] + [(32, 64, 1, 1, "affine", b) for b in ("", "in")], _conv_bounds))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [(r, s) for r in ROWS for s in r.shapes], ids=lambda p: f"{p[0].entry[4:]}:{p[0].name}-" + "x".join(str(v) for v in p[1]))
def test_no_access_outside_the_buffers(p):
    r, shape = p
    specs, call, ref = r.make(*shape)
    v, m, plain = run_case(specs, call, DEV, sync=torch.cuda.synchronize)
    assert not v, f"{r.entry} [{r.name}] {shape}:\n" + "\n".join(str(x) for x in v)
    ref(m.t)


@pytest.mark.gpu
def test_entry_point_refuses_bad_arguments_and_launches_nothing():
    _lib, ops = _sat()
    L = _lib.lib()
    c = conv_case(32, 32, 3, 1, "affine")
    widths = c["widths"][:3]
    lay = layout(widths)
    tab = table(lay)
    w16, d = _split(c)
    x, sc, sh = pack(c["xs"][:3], lay, 0.0).to(DEV), c["sc"].to(DEV), c["sh"].to(DEV)
    T = lay[2]
    y = torch.full((32, H_CONV, T), -7.0, device=DEV)
    flags = torch.zeros(3, dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()
    good = dict(x=P(x), w=P(w16), d=d, y=P(y), sc=P(sc), sh=P(sh), io=P(tab.seg_off), il=P(tab.seg_len), oo=P(tab.seg_off), B=3, ml=max(widths), cin=32, cout=32,
                H=H_CONV, Ti=T, To=T, k=3, s=1)
    bad = {
        "null x": dict(x=None), "null w_split": dict(w=None), "null y": dict(y=None), "y aliases x": dict(y=P(x)),
        "scale without shift": dict(sh=None), "shift without scale": dict(sc=None),
        "null in_off": dict(io=None), "null in_len": dict(il=None), "null out_off": dict(oo=None),
        "B = 0": dict(B=0), "B above SAT_RAGGED_MAX_SEGMENTS": dict(B=1025), "H = 0": dict(H=0), "T_in = 0": dict(Ti=0), "T_out = 0": dict(To=0),
        "max_len = 0": dict(ml=0), "max_len above T_in": dict(ml=T + 1),
        "5x5": dict(k=5), "ksize 2": dict(k=2), "stride 3": dict(s=3), "stride 0": dict(s=0),
        "the stem": dict(cin=1), "Cin = 48": dict(cin=48), "Cin = 16": dict(cin=16), "Cout = 96": dict(cout=96), "Cout = 512": dict(cout=512),
        "descale 0": dict(d=0.0), "descale < 0": dict(d=-1.0), "descale inf": dict(d=float("inf")), "descale NaN": dict(d=float("nan")),
        "an input image of 2^31 elements": dict(cin=256, H=2897, Ti=2897), "an output image of 2^31 elements": dict(cout=256, H=2897, To=2897),
        "more row tiles than the grid takes": dict(cout=256, H=65533),
    }
    for what, change in bad.items():
        a = dict(good, **change)
        status = L.sat_conv2d_f16x3_segments_f32(a["x"], a["w"], a["d"], a["y"], a["sc"], a["sh"], 1, a["io"], a["il"], a["oo"], a["B"], a["ml"], a["cin"], a["cout"],
                                                 a["H"], a["Ti"], a["To"], a["k"], a["s"], P(flags), _lib.stream())
        assert status == -1, (what, status)                                       # SAT_ERR_INVALID
        assert b"conv2d_f16x3_segments" in L.sat_last_error(), (what, L.sat_last_error())
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and flags.tolist() == [0, 0, 0]                # nothing ran
    a = good
    _lib.check(L.sat_conv2d_f16x3_segments_f32(a["x"], a["w"], a["d"], a["y"], a["sc"], a["sh"], 0, a["io"], a["il"], a["oo"], 3, a["ml"], 32, 32, H_CONV, T, T, 3, 1,
                                               None, _lib.stream()), ENTRY)
    for i in range(3):                                                            # no sticky error: a valid call is right
        assert torch.equal(tab.segment(y, i), _alone(c, 3, 1, c["xs"][i])), i


# ---- (e) no leak between segments ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_changing_one_segment_leaves_every_other_segments_bits_alone(fill):
    j = 4
    # (a stride-2 3x3: every segment's halo reaches into the gap and, without the select, into its neighbours)
    cin, cout, k, s, epi = REVERSED_CASE
    c = conv_case(cin, cout, k, s, epi)
    lin, lout = layout(c["widths"]), layout(out_widths(c["widths"], s))
    tin, tout = table(lin), table(lout)
    dirty = tuple(torch.full_like(x, fill) if i == j else x for i, x in enumerate(c["xs"]))
    fa, fb = (torch.zeros(len(c["widths"]), dtype=torch.int32, device=DEV) for _ in range(2))
    a, b = _segments(c, k, s, c["xs"], lin, tin, tout, fa, fill=fill), _segments(c, k, s, dirty, lin, tin, tout, fb, fill=fill)
    for i in range(len(c["widths"])):
        if i != j:
            assert torch.equal(tout.segment(a, i), tout.segment(b, i)), i
    assert not bool(fa.any()) and [i for i, f in enumerate(fb.tolist()) if f] == [j]


# ---- (f) the net -------------------------------------------------------------------------------------------------------------------
def _net(conv2d="f32", ragged="f32", state=None):
    import satools_amd  # noqa: F401
    from satools_amd import synthetic, xvector_resnet
    m = xvector_resnet.build()(num_speakers=10)
    m.load_state_dict(state if state is not None else synthetic.xvector_resnet_state(0, 10), strict=True)
    m = m.to(DEV)
    m.conv2d_precision, m.ragged_conv2d_precision = conv2d, ragged                  # instance attributes over the class's defaults
    return m


@pytest.fixture(scope="module")
def net16():
    """split-f16 both in `forward` and in ragged calls"""
    return _net("f16x3", "f16x3")


@pytest.fixture(scope="module")
def net32():
    return _net()


@functools.lru_cache(maxsize=None)
def net_wavs():
    from satools_amd import synthetic
    return tuple(synthetic.harm_batch([10 + i], n)[0] for i, n in enumerate(NET_SAMPLES))


@pytest.fixture(scope="module")
def rows16(net16):
    before = net16.split_fallbacks
    rows = net16.extract_batch([w.to(DEV) for w in net_wavs()])
    assert net16.last_conv2d_arithmetic == "f16x3" and net16.last_split_fallback_rows == [] and net16.split_fallbacks == before
    return rows


@pytest.mark.gpu
def test_ragged_f16x3_rows_match_the_single_f16x3_calls_the_reversed_order_and_the_padded_form(net16, rows16):
    wavs, before = net_wavs(), net16.split_fallbacks
    assert rows16.shape == (len(wavs), 256)
    back = net16.extract_batch([w.to(DEV) for w in reversed(wavs)])
    padded = torch.full((len(wavs), max(NET_SAMPLES) + 7), float("nan"))
    for i, w in enumerate(wavs):
        padded[i, :w.shape[0]] = w
    assert torch.equal(net16.extract_batch((padded.to(DEV), list(NET_SAMPLES))), rows16)          # the padded form of the argument, NaN past each end
    assert net16.last_conv2d_arithmetic == "f16x3" and net16.last_split_fallback_rows == []
    for i, w in enumerate(wavs):
        what = f"utterance {i} of {NET_SAMPLES[i]} samples"
        one = float((rows16[i] - net16(w.to(DEV))[1][0]).abs().max())
        assert net16.last_conv2d_arithmetic == "f16x3"
        rev = float((rows16[i] - back[len(wavs) - 1 - i]).abs().max())
        nrm = abs(float(rows16[i].cpu().double().norm()) - 1.0)
        print(f"{what}: vs the one-utterance f16x3 call {one:.2e}, vs the reversed batch {rev:.2e}, | norm - 1 | {nrm:.2e}")
        _note("net f16x3 row vs one-utterance f16x3 call / 1e-6", one / 1e-6, what)
        _note("net f16x3 row vs reversed order / 1e-6", rev / 1e-6, what)
        assert one < 1e-6 and rev < 1e-6 and nrm < 1e-5, what
    assert net16.split_fallbacks == before


@pytest.mark.gpu
def test_the_fixture_utterances_in_one_ragged_f16x3_call_match_the_reference(net16):
    from satools_amd import synthetic
    fx = np.load(os.path.join(GOLD, "fx_xvector_resnet.npz"))
    rows = net16.extract_batch([synthetic.harm_batch([seed], n)[0].to(DEV) for _, seed, n in FIXTURE_UTTERANCES])
    assert net16.last_conv2d_arithmetic == "f16x3" and net16.last_split_fallback_rows == []
    for i, (tag, _, _) in enumerate(FIXTURE_UTTERANCES):
        got, ref = rows[i].cpu().numpy(), fx[tag + "/xvector"][0]
        err, cos = float(np.abs(got - ref).max()), float((got.astype(np.float64) * ref).sum())
        print(f"{tag}: ragged f16x3 row max abs error vs reference {err:.2e}, cosine {cos:.7f}")
        _note("net f16x3 row vs reference fixture / 5e-6", err / 5e-6, tag)
        assert err < 5e-6 and cos > 0.999999 and abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [2, 1])
def test_a_nan_sample_gives_a_nan_row_and_changes_no_other_rows_bits(net16, bad):
    wavs = [net_wavs()[i].to(DEV) for i in (1, 3, 5)]                             # 10079, 16000 and 1280 samples
    dirty = list(wavs)
    dirty[bad] = wavs[bad].clone()
    dirty[bad][333] = float("nan")
    clean, rows = net16.extract_batch(wavs), net16.extract_batch(dirty)
    assert bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(rows[bad]).all())
    for i in range(3):
        if i != bad:
            assert torch.equal(rows[i], clean[i]), i


# ---- (g) fallback --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_row_falls_back_to_the_f32_ragged_rows():
    from satools_amd import synthetic
    sd = synthetic.xvector_resnet_state(0, 10)
    sd[ALL_FALLBACK_KEY] = sd[ALL_FALLBACK_KEY] * ALL_FALLBACK_FACTOR
    wavs = [w.to(DEV) for w in net_wavs()]
    m16, m32 = _net("f32", "f16x3", sd), _net("f32", "f32", sd)
    got, want = m16.extract_batch(wavs), m32.extract_batch(wavs)
    assert m16.last_split_fallback_rows == list(range(len(wavs))) and m16.last_conv2d_arithmetic == "f32" and m16.split_fallbacks == 1
    assert torch.equal(got, want)
    assert m32.split_fallbacks == 0 and m32.last_split_fallback_rows == [] and m32.last_conv2d_arithmetic == "f32"


def partial_wavs():
    """the utterances of the partial fallback (CPU): short harmonic ones, and at PARTIAL_CLICK one click in silence"""
    from satools_amd import synthetic
    wavs = [synthetic.harm_batch([seed], n)[0] for seed, n in PARTIAL_HARMONIC]
    click = torch.zeros(PARTIAL_CLICK_SAMPLES)
    click[PARTIAL_CLICK_SAMPLES // 2] = 0.5
    wavs.insert(PARTIAL_CLICK, click)
    return wavs


def partial_state():
    from satools_amd import synthetic
    sd = synthetic.xvector_resnet_state(0, 10)
    sd["sequence_network.bn1.weight"] = sd["sequence_network.bn1.weight"] * PARTIAL_STEM_SCALE
    return sd


@pytest.mark.gpu
def test_only_the_utterance_outside_the_range_falls_back():
    sd = partial_state()
    wavs = [w.to(DEV) for w in partial_wavs()]
    m16, m32 = _net("f32", "f16x3", sd), _net("f32", "f32", sd)
    got, want = m16.extract_batch(wavs), m32.extract_batch(wavs)
    assert m16.last_split_fallback_rows == [PARTIAL_CLICK] and m16.last_conv2d_arithmetic == "f16x3+f32" and m16.split_fallbacks == 1
    assert torch.equal(got[PARTIAL_CLICK], want[PARTIAL_CLICK])                   # the f32 ragged row of that utterance
    others = [i for i in range(len(wavs)) if i != PARTIAL_CLICK]
    alone = m16.extract_batch([wavs[i] for i in others])                          # the others keep their f16x3 bits
    assert m16.last_split_fallback_rows == [] and m16.last_conv2d_arithmetic == "f16x3" and m16.split_fallbacks == 1
    assert torch.equal(got[others], alone)
    assert not torch.equal(got[others], want[others])                             # (and those are not the f32 bits)
    assert bool(torch.isfinite(got).all())


# ---- (h) the default is unchanged ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_with_the_ragged_attribute_at_f32_extract_batch_gives_the_existing_rows(net32):
    wavs = [w.to(DEV) for w in net_wavs()]
    clean = net32.extract_batch(wavs)
    assert net32.last_conv2d_arithmetic == "f32" and net32.last_split_fallback_rows == []
    m = _net("f16x3", "f32")
    m(wavs[0])
    assert m.last_conv2d_arithmetic == "f16x3" and m.ragged_conv2d_precision == "f32"
    rows = m.extract_batch(wavs)
    assert m.last_conv2d_arithmetic == "f32" and m.last_split_fallback_rows == [] and m.split_fallbacks == 0
    assert torch.equal(rows, clean)
