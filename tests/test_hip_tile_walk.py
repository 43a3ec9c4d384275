"""The persistent kernels where a block takes a second tile: resblock_pair16_kernel, mrf16_kernel, pair32s_kernel, pairw_kernel, ups2_kernel,
conv1d_f16x3_ring16_kernel in all its forms and gemm_f16x3_walk16_kernel.  What is fragile in them — the next tile's image requested while this
one computes, the barrier that frees the previous tile's LDS, the double-buffer flip, the descriptor rebuilt when the walk crosses into another
utterance, empty regions, the rotating job order — happens from a block's second tile on, and the shapes of tests/test_hip_parity.py and of the
table of tests/test_hip_bounds.py stop short of it (tests/test_walk_plan_host.py::test_the_kernel_level_shapes_of_the_older_tests_walk_nowhere).

The shapes are the catalogue of tests/test_walk_plan_host.py, whose properties are asserted there from the plan (tests/walk_plan.py).  Each is checked
    (a) as a row of tests/test_hip_bounds.py is: the call under tests/moat.py's two fills and on plain tensors (W, R/U, E — E and R/U are also the
        determinism check: three runs on fresh outputs, equal bits), the dispatch name, and the row's own float64 reference at the row's own bound
        (2e-5 pair16 and mrf16; 1e-5 pair32s, pairw, ups2; 3e-5 ring conv f16x3 and the GEMM; 1e-4 of the scale SAT_CONV_F16F8R; the upsampler rows 4e-6)
    (b) bit for bit against the same tiles computed by blocks that take ONE tile: the output of a tile does not depend on which block computed it,
        and tile boundaries are multiples of the width inside each utterance.  Slot kernels: consecutive sub-batches of at most 8 * cap tiles
        (crossing, even); crops [a, a + L) of the long utterance, a a multiple of the width, compared further than the staged halo from a crop
        edge.  Ring conv: the same call under convring_blocks = 8 and under the default grid.  GEMM: gemm_f16x3_ring16_kernel (one tile per block).
A failure names the kernel, the form and the first tile that differs.  Needs a real MI355X: run with `-m gpu`."""
import ctypes as C
import math
import time

import pytest
import torch
import torch.nn.functional as F

import test_hip_bounds as hb
import test_walk_plan_host as cat
import walk_plan as wp
from moat import plain_tensors, run_case

DEV = "cuda"
pytestmark = pytest.mark.gpu
RINGFAM, F8FAM = "conv1d_f16x3_ring16_kernel", hb.F8FAM
WALK = (("convring", 33, 1), ("convring_blocks", cat.RING_BLOCKS, 0))          # the ring whatever the number of tiles, on 8 blocks
UNWALKED = (("convring", 33, 1),)


def cu_count():
    n = C.c_int(0)
    hb._ok(hb._L().sat_device_info(None, 0, C.byref(n)), "sat_device_info")
    assert n.value >= 8
    return n.value


# ---- the calls ----------------------------------------------------------------------------------------------------------------------
def _pair(Cc, k, dil, kernel, bound, **kw):
    return lambda B, T, **given: hb.pair_case(B, T, Cc, k, dil, planes=True, family=kernel, bound=bound, **kw, **given)


# (family, form) -> (kernel, builder(B, T, x=, acc0=), staged halo in input columns, output columns per input column)
SLOT_CALLS = {
    ("pair16", 3): ("resblock_pair16_kernel", _pair(16, 3, 1, "resblock_pair16_kernel", 2e-5), 16 + 2 * 1, 1),          # FP_OFF + (k - 1) * dil
    ("pair16", 7): ("resblock_pair16_kernel", _pair(16, 7, 3, "resblock_pair16_kernel", 2e-5), 16 + 6 * 3, 1),
    ("pair16", 11): ("resblock_pair16_kernel", _pair(16, 11, 5, "resblock_pair16_kernel", 2e-5, no_y=True), 16 + 10 * 5, 1),
    ("mrf16", None): ("mrf16_kernel", lambda B, T, x=None, acc0=None: hb.mrf_case(B, T, 3, 1, x=x), 64, 1),                 # MRF_HP
    ("pair32s", 8): ("pair32s_kernel", _pair(32, 3, 5, "pair32s_kernel", 1e-5), 2 * (5 + 1) // 2, 1),                      # (k - 1) * (dil + 1) / 2
    ("pair32s", 4): ("pair32s_kernel", _pair(32, 3, 1, "pair32s_kernel", 1e-5, accum=True, options=(("pair32s_waves", 4, 8),)), 2 * (1 + 1) // 2, 1),
    ("pairw", 32): ("pairw_kernel", _pair(32, 7, 3, "pairw_kernel", 1e-5, no_y=True), 6 * (3 + 1) // 2, 1),
    ("pairw", 64): ("pairw_kernel", _pair(64, 3, 3, "pairw_kernel", 1e-5, options=(("pair64w", 1, 0),)), 2 * (3 + 1) // 2, 1),
    ("ups2", 32): ("ups2_kernel", lambda B, T, x=None, acc0=None: hb.ups2_case(B, T, 32, x=x), 2, 2),
    ("ups2", 64): ("ups2_kernel", lambda B, T, x=None, acc0=None: hb.ups2_case(B, T, 64, x=x), 2, 2),
}
assert set(SLOT_CALLS) == set(cat.SLOT)


def _outputs(case):
    return [s.name for s in case.specs if s.role in ("out", "inout")]


def _call_checked(case):
    """the case's call, followed by the assertion that the dispatch picked the kernel this file is about"""
    def call(t):
        case.call(t)
        name = hb._L().sat_last_dispatch_name().decode().split("<")[0].strip()
        assert name == case.family, f"meant to hit {case.family}, the dispatch picked {name}"
    return call


def run_moat(case, what):
    """(a): W, R/U, E and the case's float64 reference; -> the outputs of the plain run"""
    with hb._options(case.options):
        v, m, plain = run_case(case.specs, _call_checked(case), DEV, sync=torch.cuda.synchronize)
    assert not v, f"{what}:\n" + "\n".join(str(x) for x in v)
    t0 = time.perf_counter()
    with hb._options(case.options):          # (a hi-only conv row repeats its call inside the reference)
        case.ref(m.t)
    print(f"TILEWALK {what}: float64 reference and comparison {time.perf_counter() - t0:.2f} s")
    return {n: plain[n] for n in _outputs(case)}


def run_plain(case, options=None):
    t = plain_tensors(case.specs, DEV)
    with hb._options(case.options if options is None else options):
        _call_checked(case)(t)
        torch.cuda.synchronize()
    return {n: t[n] for n in _outputs(case)}


def _tdim(t):
    return -1 if t.dim() == 3 else -2          # [B][C][T] f32; planes [B][chunk][2][2][T][8] and their sidecar [B][chunk][2][T][16]


def _cols(t, lo, hi):
    return t.narrow(_tdim(t), lo, hi - lo)


def _first_difference(a, b):
    """(utterance, column) of the first element that differs"""
    d = (a != b)
    d = d.movedim(_tdim(a), 1).flatten(2).any(-1)          # [B][T]
    u, q = d.nonzero()[0].tolist()
    return u, q


def _where(family, kw, B, T, u, q, up):
    width, _ = wp.slot_form(family, **kw)
    tile = (u, q // up // width)
    for blk, mine in enumerate(wp.slot_plan(family, B, T, **kw)):
        if tile in mine:
            return f"utterance {u}, output column {q}: tile {tile[1]} of the utterance, tile number {mine.index(tile)} of the walk of block {blk} (of {len(mine)})"
    return f"utterance {u}, output column {q}"


# ---- slot kernels -----------------------------------------------------------------------------------------------------------------
_SLOT_IDS = [(family, f, kind) for (family, f) in cat.SLOT for kind in ("long", "crossing", "even")]
_LAST = {}          # the walked outputs of the case (a) ran last, for (b) right behind it


def _walked(family, f, kind):
    key = (family, f, kind)
    if _LAST.get("key") != key:
        _LAST.clear()
        B, T = cat.SLOT[(family, f)][kind]
        kernel, make, halo, up = SLOT_CALLS[(family, f)]
        case = make(B, T)
        assert case.family == kernel
        _LAST.update(key=key, case=case, out=None)
    return _LAST


@pytest.mark.parametrize("family,f,kind", _SLOT_IDS, ids=lambda v: str(v))
def test_walked_slot_kernel_stays_inside_its_buffers_and_matches_float64(family, f, kind):
    """(a) and (c)"""
    w = _walked(family, f, kind)
    p = wp.slot_props(family, *cat.SLOT[(family, f)][kind], **cat.form_kw(family, f))
    assert p["walk_steps"] > 0 and max(p["counts"]) == (3 if kind == "crossing" else 2)
    w["out"] = run_moat(w["case"], f"{SLOT_CALLS[(family, f)][0]} {f or ''} {kind} {cat.SLOT[(family, f)][kind]}")


@pytest.mark.parametrize("family,f,kind", _SLOT_IDS, ids=lambda v: str(v))
def test_walked_slot_kernel_gives_the_bits_of_one_tile_per_block(family, f, kind):
    """(b)"""
    w = _walked(family, f, kind)
    kw = cat.form_kw(family, f)
    B, T = cat.SLOT[(family, f)][kind]
    kernel, make, halo, up = SLOT_CALLS[(family, f)]
    width, cap = wp.slot_form(family, **kw)
    walked = w["out"] if w["out"] is not None else run_plain(w["case"])
    data = w["case"].data
    x, acc0 = data["x"], data.get("acc0")
    what = f"{kernel} {f or ''} {kind} B = {B}, T = {T}"
    if kind == "long":
        for a, L in cat.crops(family, **kw):
            sub = make(1, L, x=x[:, :, a:a + L].contiguous(), acc0=None if acc0 is None else acc0[:, :, a:a + L].contiguous())
            assert wp.slot_props(family, 1, L, **kw)["walk_steps"] == 0
            got = run_plain(sub)
            lo, hi = (halo if a > 0 else 0) * up, (L - (halo if a + L < T else 0)) * up
            assert hi - lo >= width * up
            for n, g in got.items():
                want, g = _cols(walked[n], a * up + lo, a * up + hi), _cols(g, lo, hi)
                if not torch.equal(g, want):
                    u, q = _first_difference(g, want)
                    raise AssertionError(f"{what}: {n} differs from the crop [{a}, {a + L}) at " + _where(family, kw, B, T, 0, a * up + lo + q, up))
        _LAST.clear()
        return
    step = cat.sub_batch(family, B, T, **kw)
    assert step * wp.ceil_div(T, width) <= 8 * cap
    for b0 in range(0, B, step):
        n_sub = min(step, B - b0)
        sub = make(n_sub, T, x=x[b0:b0 + n_sub].contiguous(), acc0=None if acc0 is None else acc0[b0:b0 + n_sub].contiguous())
        got = run_plain(sub)
        for n, g in got.items():
            want = walked[n][b0:b0 + n_sub]
            if not torch.equal(g, want):
                u, q = _first_difference(g, want)
                raise AssertionError(f"{what}: {n} differs from the sub-batch [{b0}, {b0 + n_sub}) at " + _where(family, kw, B, T, b0 + u, q, up))
    _LAST.clear()


# ---- the ring conv ------------------------------------------------------------------------------------------------------------------
def rotating_jobs_case(B, T, options=()):
    """three independent ring jobs in one sat_conv1d_multi_f32 launch (the first convs of the three branches of an MRF block: 3 / 7 / 11 taps on the same
    planes, each to planes of its own): no job reads what another writes, so the launch rotates the job order with the region number"""
    _, ops, _ = hb._sat()
    Cc, ks, dils = 128, (3, 7, 11), (1, 3, 5)
    c = hb.Case(family=RINGFAM, options=tuple(options))
    x = hb.rand(B, Cc, T, seed=T)
    xs = ops.act_split(x.to(DEV), 0.1)
    ws = [hb.rand(Cc, Cc, k, seed=10 + k, scale=(k * Cc) ** -0.5) for k in ks]
    bs = [hb.rand(Cc, seed=20 + k) for k in ks]
    attrs = []
    c.inp("x_split", xs)
    c.untouched("x", (B, Cc, T))
    c.untouched("y", (B, Cc, T))
    for j, k in enumerate(ks):
        wp_, a = hb._pack(ws[j], 1)
        attrs.append(a)
        c.inp(f"w{j}", wp_)
        c.inp(f"b{j}", bs[j])
        c.out(f"y_split{j}", (B, Cc // 16, 2, 2, T, 8), hb.F16)

    def call(t):
        ops.conv1d_multi([(t["x"], hb._attrs(t[f"w{j}"], attrs[j]), Cc, k,
                           dict(bias=t[f"b{j}"], dilation=dils[j], pad_left=dils[j] * (k - 1) // 2, mode=1, x_split=t["x_split"], y_split=t[f"y_split{j}"],
                                y_split_slope=0.1, no_y=True, out=t["y"])) for j, k in enumerate(ks)])
    c.call = call

    def ref(t):          # the single convs' bar: 3e-5, and what the planes lose of lrelu(v)
        pre = ops.unsplit(xs).double().cpu()
        for j, k in enumerate(ks):
            want = F.leaky_relu(F.conv1d(pre, ws[j].double(), bs[j].double(), dilation=dils[j], padding=dils[j] * (k - 1) // 2), 0.1)
            hb.bounded(f"rotating ring job {j}", ops.unsplit(t[f"y_split{j}"]), want, 3e-5 + 2.0 ** -21 * want.abs())
    c.ref = ref
    return c


def _conv(cin, cout, k, **kw):
    return lambda B, T, options, **given: hb.conv_case(B, T, cin, cout, k, x_planes=True, slope=0.1, options=options, **kw, **given)


def _ups(cin, cout, **kw):
    return lambda B, T, options: hb.ups_case(B, T, cin, cout, 8, 4, mode=1, planes=True, grouped=True, family=RINGFAM, options=options, bound=4e-6, **kw)


# form -> (builder(B, T, options), extra options, COLS, n_rt, jobs): the rows of tests/test_hip_bounds.py, and what they leave out
RING_CALLS = {
    "256x160 f16x3": (_conv(256, 256, 7, dil=3, mode=1, y_planes=True, res="planes", accum=True, accum_div=3.0, family=RINGFAM), (), 160, 1, 1),
    "128x320 f16x3": (_conv(128, 128, 3, dil=5, mode=1, y_planes=True, no_y=True, sidecar=True, family=RINGFAM), (), 320, 1, 1),
    "128x320 f16x3 hi-only planes": (_conv(128, 128, 11, mode=1, y_planes=True, no_y=True, sidecar=True, hi_only=True, family=RINGFAM), (), 320, 1, 1),
    "256x160 F8": (_conv(256, 256, 11, dil=5, mode=3, y_planes=True, res="planes", sidecar=True, bound=1e-4, family=F8FAM), (), 160, 1, 1),
    "128x320 F8": (_conv(128, 128, 3, mode=3, y_planes=True, no_y=True, sidecar=True, bound=1e-4, family=F8FAM), (), 320, 1, 1),
    "128x320 f16x3 for 256 rows (convring_wr 1)": (_conv(256, 256, 7, dil=3, mode=1, y_planes=True, res="planes", accum=True, accum_div=3.0, family=RINGFAM),
                                                   (("convring_wr", 1, 0),), 320, 2, 1),
    "128x320 F8 for 256 rows (convring_wr 2)": (_conv(256, 256, 11, dil=5, mode=3, y_planes=True, res="planes", sidecar=True, bound=1e-4, family=F8FAM),
                                                (("convring_wr", 2, 0),), 320, 2, 1),
    "256x160 two row tiles (C_out 512)": (_conv(256, 512, 3, mode=1, y_planes=True, family=RINGFAM), (), 160, 2, 1),
    "upsampler UPS_MASK_K8": (_ups(256, 128, mask=0x30c), (), 160, 2, 1),
    "upsampler generic mask": (_ups(128, 64, mask=0, sidecar=True), (), 160, 1, 1),
    "three rotating jobs": (lambda B, T, options: rotating_jobs_case(B, T, options), (), 320, 1, 3),
}
# (B, column tiles per utterance): n_ct * B = 9 and 17 (the catalogue's entries with one row tile; with two the same shapes give 4 and 6 regions per block)
RING_SHAPES = [(3, 3), (1, 17)]
assert set(cat.RING.values()) <= {(n_rt, n_ct, B, njobs, njobs > 1) for _, _, _, n_rt, njobs in RING_CALLS.values() for B, n_ct in RING_SHAPES}


@pytest.mark.parametrize("shape", RING_SHAPES, ids=lambda v: "B%d-%dtiles" % v)
@pytest.mark.parametrize("form", list(RING_CALLS))
def test_ring_conv_on_eight_blocks(form, shape):
    """(a) under convring_blocks = 8 and (b) against the default grid, where these shapes have one region per block"""
    make, extra, cols, n_rt, njobs = RING_CALLS[form]
    B, n_ct = shape
    T = (n_ct - 1) * cols + 1          # the last column tile one column wide
    n_vb = wp.ring_regions(n_rt, n_ct, B)
    walk =wp.plan("ring", n_rt=n_rt, n_ct=n_ct, B=B, njobs=njobs, rotate=njobs > 1, grid=wp.ring_grid(n_vb, cu_count(), cat.RING_BLOCKS))
    assert len(walk) == 8 and min(len(b) for b in walk) >= 2 * njobs, "more than one region per block"
    assert wp.ring_grid(n_vb, cu_count()) == n_vb, "one region per block at the default grid"
    case = make(B, T, WALK + extra)
    walked = run_moat(case, f"ring conv [{form}] B = {B}, T = {T} on 8 blocks")
    plain = run_plain(case, UNWALKED + extra)
    for n in walked:
        if not torch.equal(walked[n], plain[n]):
            u, q = _first_difference(walked[n], plain[n])
            raise AssertionError(f"ring conv [{form}] B = {B}, T = {T}: {n} on 8 blocks differs from the default grid at utterance {u}, column {q} "
                                 f"(column tile {q // cols if 'upsampler' not in form else q // 4 // cols})")


def test_ring_conv_walks_at_the_default_grid():
    """C = 128, 3 taps, CUs + 1 column tiles: n_vb = CUs + 8 regions on CUs blocks, blocks 0..7 take a second region (seven of them empty).  Bits
    against sub-batches of no more regions than blocks (the float64 check of this form is made on 8 blocks)"""
    cus = cu_count() // 8 * 8
    print(f"TILEWALK the device has {cu_count()} CUs")
    make = RING_CALLS["128x320 f16x3"][0]
    B, T = cus + 1, 300
    n_vb = wp.ring_regions(1, 1, B)
    grid = wp.ring_grid(n_vb, cus)
    assert n_vb == cus + 8 > grid == cus
    walk = wp.plan("ring", n_rt=1, n_ct=1, B=B, grid=grid)
    assert sorted({len(b) for b in walk}) == [1, 2] and sum(len(b) == 2 for b in walk) == 8
    case = make(B, T, UNWALKED)
    walked = run_plain(case)
    x = case.data["x"]
    step = cus // 2
    for b0 in range(0, B, step):
        n_sub = min(step, B - b0)
        assert wp.ring_regions(1, 1, n_sub) <= cus
        got = run_plain(make(n_sub, T, UNWALKED, x=x[b0:b0 + n_sub].contiguous()))
        for n, g in got.items():
            assert torch.equal(g, walked[n][b0:b0 + n_sub]), f"ring conv 128x320 at the default grid: {n} differs in utterances [{b0}, {b0 + n_sub})"
    again = run_plain(case)
    assert all(torch.equal(again[n], walked[n]) for n in walked)


# ---- the persistent GEMM ------------------------------------------------------------------------------------------------------------
def _gemm_shapes():
    """(name, cin, cout, B, T).  n_vb = 8 * n_rt * ceil(n_ct * B / 8) is a multiple of 8 * n_rt = 64 at cout = 1024: the fewest regions above the grid
    are the next multiple of 64 (CUs + 64 on 256 CUs: a quarter of the blocks take 2 regions, the others 1), not CUs + 8; that count has cout = 128"""
    cus = cu_count() // 8 * 8
    uneven = (cus // 64 + 1) * 64
    even = math.lcm(64, cus)
    even *= -(-2 * cus // even)
    return cus, [("uneven", 256, 1024, uneven // 64 * 8 - 5, 255, uneven), ("even", 256, 1024, even // 64 * 4 - 1, 500, even),
                 ("CUs + 8", 256, 128, cus + 3, 255, cus + 8)]


@pytest.mark.parametrize("which", ["uneven", "even", "CUs + 8"])
def test_persistent_gemm_walks_more_regions_than_blocks(which):
    """gemm_f16x3_walk16_kernel with n_vb above the grid, every kind of epilogue it carries: the bits of gemm_f16x3_ring16_kernel (gemm_walk 0), and
    float64 at 3e-5 for the plain kind — the assertions of tests/test_hip_parity.py::test_persistent_ring_gemm_gives_the_bits_of_the_ring_gemm"""
    _, ops, packing = hb._sat()
    cus, shapes = _gemm_shapes()
    name, cin, cout, B, T, want_vb = next(s for s in shapes if s[0] == which)
    n_rt, n_ct = wp.ceil_div(cout, wp.WALK_TILE[0]), wp.ceil_div(T, wp.WALK_TILE[1])
    n_vb = wp.ring_regions(n_rt, n_ct, B)
    grid = wp.walk_grid(n_vb, cus)
    assert n_vb == want_vb > grid == cus
    for njobs in (1, 3):
        counts = sorted({len(b) for b in wp.plan("gemm_walk16", n_rt=n_rt, n_ct=n_ct, B=B, njobs=njobs, grid=grid)})
        assert counts == ([2 * njobs] if which == "even" else [njobs, 2 * njobs])
    x = hb.rand(B, cin, T, seed=1).to(DEV)
    xs = ops.act_split(x, 1.0)
    ws = [hb.rand(cout, cin, 1, seed=10 + j, scale=cin ** -0.5) for j in range(3)]
    wps = [packing.pack_conv_weight_f16x3(w.to(DEV)) for w in ws]
    bs = [hb.rand(cout, seed=20 + j).to(DEV) for j in range(3)]
    res = hb.rand(B, cout, T, seed=30).to(DEV)
    tp = (T + 63) // 64 * 64

    def run(kind, multi):
        if kind == "qkv":
            qs, ks = ops.split_like(B, cout, T, DEV).zero_(), ops.split_like(B, cout, T, DEV).zero_()
            v = torch.zeros(B, cout, tp, device=DEV)
            jobs = [(x, wps[0], cout, 1, dict(bias=bs[0], mode=1, x_split=xs, y_split=qs, y_split_slope=1.0, no_y=True)),
                    (x, wps[1], cout, 1, dict(bias=bs[1], mode=1, x_split=xs, y_split=ks, y_split_slope=1.0, no_y=True)),
                    (x, wps[2], cout, 1, dict(bias=bs[2], mode=1, x_split=xs, out=v[:, :, :T]))]
            if multi:
                ops.conv1d_multi(jobs)
            else:
                for (xx, w, c, k, kw) in jobs:
                    ops.conv1d(xx, w, c, k, **kw)
            return (qs, ks, v)
        if kind == "plain":
            return (ops.conv1d(x, wps[0], cout, 1, bias=bs[0], mode=1, x_split=xs),)
        if kind == "res":
            return (ops.conv1d(x, wps[0], cout, 1, bias=bs[0], mode=1, x_split=xs, res=res),)
        ys = ops.split_like(B, cout, T, DEV).zero_()
        ops.conv1d(x, wps[0], cout, 1, bias=bs[0], gelu=True, mode=1, x_split=xs, y_split=ys, y_split_slope=1.0, no_y=True)
        return (ys,)

    for kind in ("plain", "res", "gelu_planes", "qkv"):
        with hb._options((("gemm_walk", 0, 1),)):
            old = run(kind, False)
            assert "ring16" in hb._L().sat_last_dispatch_name().decode()
        with hb._options((("gemm_walk", 3, 1),)):
            new = run(kind, True)
            name = hb._L().sat_last_dispatch_name().decode()
            assert "walk16" in name, (kind, name)
            again = run(kind, True)
        torch.cuda.synchronize()
        for a, b, c in zip(old, new, again):
            assert torch.equal(a, b), f"gemm_f16x3_walk16_kernel [{kind}] {which}: B = {B}, T = {T}, {cin} -> {cout} differs from gemm_f16x3_ring16_kernel"
            assert torch.equal(b, c), f"gemm_f16x3_walk16_kernel [{kind}] {which}: two runs differ"
        if kind == "plain" and cout == 1024:
            ref = F.conv1d(ops.unsplit(xs).double().cpu(), ws[0].double(), bs[0].double().cpu())
            hb.bounded(f"gemm_f16x3_walk16_kernel plain {which}", new[0], ref, 3e-5)


# ---- the whole generator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f16f8r"])
def test_generator_on_eight_ring_blocks_gives_the_same_waveform(precision):
    """sat_hifigan_forward_f32 on the synthetic generator, B = 3, T = 25, every thick conv on the ring (convring 33; f16f8r forced): under
    convring_blocks = 8 the forward's own multi-branch launches walk — the bits of the default grid"""
    g = hb._generator(precision)
    x = hb.rand(3, g.imput_dim, 25, seed=25).to(DEV)
    g.set_force_f8(int(precision == "f16f8r"))
    try:
        with hb._options(WALK):
            y8 = g.forward_resnet(x).clone()
            ran = g.last_arithmetic
            again = g.forward_resnet(x).clone()
        with hb._options(UNWALKED):
            y0 = g.forward_resnet(x).clone()
            assert g.last_arithmetic == ran
    finally:
        g.set_force_f8(0)
    torch.cuda.synchronize()
    assert ran.startswith(precision), (ran, precision)
    assert bool(torch.isfinite(y0).all()) and torch.equal(y8, again)
    assert torch.equal(y8, y0), f"{precision} generator: the waveform on 8 ring blocks differs from the default grid at sample {int((y8 != y0).flatten().nonzero()[0])}"
