"""The epilogue of sat_conv1d_f32 under every option set ops.conv1d exposes, on one small carrier shape per epilogue implementation and dispatch
branch (csrc/conv_common.h conv_epilogue fast and general path, conv_epilogue16; csrc/conv_ring16.hip ring_epilogue; csrc/gemm_walk16.hip), against
the float64 restatement of the descriptor in tests/ref64_conv.py with its running bound (E0 = 3e-5, the bar of tests/test_hip_parity.py, moved through
every step; no figure here is fitted to the device).

Per call: |y - want| <= bound elementwise; the same on ops.unsplit(y_split) with the plane term; y_split == act_split(y) bit for bit where both are
written; with no_y the f32 buffer keeps its sentinel.  A refusal (SatError) is accepted only where REFUSED names it, with the message of its
SAT_REQUIRE; a listed set that is served fails too.  The kernel family that served every accepted call is recorded: a carrier meant for a family
that carries a SUBSET of the epilogue (the LDS-DMA conv ring, the persistent GEMM walk, the lean tile) must see that family serve some sets and
another family serve the ones it declines, all within the same bound.

The recipes that reach each family (shapes, sat_conv_set_option switches) are those of the conv_rows of tests/test_hip_bounds.py.  Every call is a
valid call on fully sized buffers.  The module imports without a GPU: tests/test_ref64_conv.py walks CARRIERS on the CPU."""
from dataclasses import dataclass

import pytest
import torch

import ref64_conv as R

DEV = "cuda"
B = 2
SENTINEL = -7.25          # what an f32 output holds before a call that must not write it
RING = (("convring", 33, 1),)


@dataclass(frozen=True)
class Carrier:
    name: str
    family: str               # the kernel the shape and the switches are meant to reach
    cin: int
    cout: int
    k: int                    # taps (up > 1: of the ConvTranspose1d)
    T: int
    mode: int = 0             # SAT_CONV_F32 / SAT_CONV_F16X3
    dil: int = 1
    stride: int = 1
    pads: tuple = None        # default: 'same'
    groups: int = 1
    up: int = 1
    x_planes: bool = False
    wrap: int = 0
    options: tuple = ()       # (name, value, default) of sat_conv_set_option
    restricted: bool = False  # `family` carries a subset of the epilogue: some sets must fall through to another family

    @property
    def halo(self):
        return self.dil * (self.k - 1)

    @property
    def padding(self):
        return self.pads if self.pads is not None else (self.halo // 2, self.halo - self.halo // 2)

    @property
    def t_out(self):
        if self.up > 1:
            return self.T * self.up
        if self.wrap:
            return self.T
        pl, pr = self.padding
        return (self.T + pl + pr - self.halo - 1) // self.stride + 1


MFMA, F16X3, LEAN = "conv1d_mfma_kernel", "conv1d_f16x3_kernel", "conv1d_f16x3_planes_lean_kernel"
CARRIERS = [
    # exact f32: the three tile shapes, a strided conv, the polyphase rows of two upsamplers (conv_epilogue's general path)
    Carrier("f32 64x256 k3 dilated", MFMA, 24, 40, 3, 261, dil=2),
    Carrier("f32 128x32 504->512 k7", MFMA, 504, 512, 7, 37),
    Carrier("f32 32x512 groups 4", MFMA, 32, 48, 3, 517, groups=4),
    Carrier("f32 stride 2 k2", MFMA, 48, 40, 2, 267, stride=2, pads=(0, 0)),
    Carrier("f32 up 2", MFMA, 32, 24, 4, 261, up=2),
    Carrier("f32 up 4 k8", MFMA, 32, 24, 8, 37, up=4),
    # split-f16 from an f32 input
    Carrier("f16x3 f32-in 32 rows k3", F16X3, 16, 16, 3, 517, mode=1),
    Carrier("f16x3 f32-in k7 half-width tile", F16X3, 24, 48, 7, 133, mode=1),
    Carrier("f16x3 f32-in k7 full tile", F16X3, 24, 48, 7, 261, mode=1, options=(("half_tile7", 0, 1),)),
    Carrier("f16x3 f32-in k2 40 rows", F16X3, 48, 40, 2, 261, mode=1),
    Carrier("f16x3 f32-in up 2", F16X3, 32, 24, 4, 261, mode=1, up=2),
    # split-f16 on planes
    Carrier("planes 64x256 k7 (lean off)", F16X3, 64, 48, 7, 261, mode=1, x_planes=True, options=(("lean7", 0, 1),)),
    Carrier("planes lean k7", LEAN, 64, 48, 7, 261, mode=1, dil=3, x_planes=True, restricted=True),
    Carrier("planes 32 rows k11", F16X3, 32, 32, 11, 517, mode=1, x_planes=True),
    Carrier("planes k3 half-width tile", F16X3, 64, 48, 3, 133, mode=1, x_planes=True),
    # 1x1 on planes: the conv tile and the four GEMM kernels (256-column tiles are taken where they pad the time axis no more than 128-column ones)
    Carrier("k1 conv tile (k1_gemm 0)", F16X3, 64, 144, 1, 261, mode=1, x_planes=True, options=(("k1_gemm", 0, 3),)),
    Carrier("k1 128x128 gemm (k1_gemm 1)", "conv1d_f16x3_k1_kernel", 64, 144, 1, 133, mode=1, x_planes=True, options=(("k1_gemm", 1, 3),)),
    Carrier("k1 ring gemm 32x32x16 (k1_gemm 2)", "gemm_f16x3_ring_kernel", 128, 256, 1, 400, mode=1, x_planes=True, options=(("k1_gemm", 2, 3),)),
    Carrier("k1 ring16 gemm T 255", "gemm_f16x3_ring16_kernel", 128, 256, 1, 255, mode=1, x_planes=True),
    Carrier("k1 ring16 gemm T 256", "gemm_f16x3_ring16_kernel", 128, 256, 1, 256, mode=1, x_planes=True),
    Carrier("k1 walk gemm (gemm_walk 3)", "gemm_f16x3_walk16_kernel", 128, 256, 1, 400, mode=1, x_planes=True, options=(("gemm_walk", 3, 1),), restricted=True),
    Carrier("k1 wrapped (x_wrap_channels)", "gemm_f16x3_ring16_kernel", 192, 128, 1, 261, mode=1, x_planes=True, wrap=128),
    # the LDS-DMA conv ring: one 128 x 320 tile + 3
    Carrier("conv ring 128 rows k3", "conv1d_f16x3_ring16_kernel", 128, 128, 3, 323, mode=1, x_planes=True, options=RING, restricted=True),
]
# gemm_f16x3_ring16_kernel is the fourth kernel with a predicate of its own, but ring16_supports (csrc/gemm_ring.hip) holds no clause on an epilogue
# OPTION: conv_epilogue16 carries the whole epilogue, so no set of the lattice is declined by it.  It is what the walk's declined sets fall through to
# (the walk carrier sees both), and test_ring16_declines_e4m3_planes takes the one descriptor field outside the lattice that it does decline.

# ---- the refusals conv1d_prepare documents, in its order (csrc/conv1d_api.hip): the first entry that applies is the one expected ----------------
PLANES_RES = ("planes", "planes scaled")
REFUSED = [
    ("split planes in exact-f32 mode", lambda c, o: c.mode == 0 and (o.out != "f32" or o.res in PLANES_RES),
     "conv1d: split planes need a split-f16 mode"),
    ("res_split on polyphase rows, groups or C_out % 16 != 0", lambda c, o: o.res in PLANES_RES and (c.up > 1 or c.groups > 1 or c.cout % 16 != 0),
     "conv1d(f16x3): res_split needs up 1, groups 1, C_out % 16 == 0, no f32 res"),
    ("planes out of a polyphase conv with an f32 input", lambda c, o: o.out != "f32" and c.up > 1,
     "conv1d(f16x3): up > 1 with y_split needs split-plane input, no_y"),
    ("planes out with groups or C_out % 16 != 0", lambda c, o: o.out != "f32" and (c.groups > 1 or c.cout % 16 != 0),
     "conv1d(f16x3): y_split / no_y need up 1, groups 1, C_out % 16 == 0"),
    ("no_y with accum", lambda c, o: o.out == "planes" and o.accum in ("accum", "accum div"), "conv1d: no_y with accum"),
]


def refusal(c, o):
    """the SAT_REQUIRE message this option set must be refused with on this carrier, or None"""
    for _, applies, msg in REFUSED:
        if applies(c, o):
            return msg
    return None


def host_inputs(c):
    """x, the weight in torch layout (up > 1: the ConvTranspose1d weight) and the epilogue's operands: float32 on the CPU, the same for both test files"""
    g = torch.Generator().manual_seed(1000 + c.T + c.cin)
    x = torch.randn(B, c.wrap or c.cin, c.T, generator=g)
    if c.up > 1:
        w = torch.randn(c.cin, c.cout, c.k, generator=g) * (c.cin * c.k / c.up) ** -0.5
    else:
        w = torch.randn(c.cout, c.cin // c.groups, c.k, generator=g) * (c.cin // c.groups * c.k) ** -0.5
    return x, w, R.epilogue_inputs(B, c.cout, c.t_out, seed=c.T)


def pre_sum(c, pre, w, in_lrelu, dtype=torch.float64):
    return R.pre_sum(pre, w, dilation=c.dil, stride=c.stride, pads=c.padding, groups=c.groups, in_slope=R.IN_SLOPE if in_lrelu else None, up=c.up,
                     up_padding=(c.k - c.up) // 2, wrap=c.wrap, t_q=c.t_out, dtype=dtype)


# ---- the device side ---------------------------------------------------------------------------------------------------------------------------
def _sat():
    import satools_amd  # noqa: F401
    from satools_amd import _lib, ops, packing
    return _lib, ops, packing


class _options:
    """sat_conv_set_option for the duration of a with-block, restored afterwards (conv_option of tests/test_hip_parity.py)"""

    def __init__(self, opts):
        self.opts = opts

    def _set(self, i):
        _lib = _sat()[0]
        for o in self.opts:
            _lib.check(_lib.lib().sat_conv_set_option(o[0].encode(), o[i]), "sat_conv_set_option")

    def __enter__(self):
        self._set(1)

    def __exit__(self, *a):
        self._set(2)


_STATE = {}          # carrier name -> what every case of the carrier shares
TABLE = {}           # carrier name -> {"families": {full kernel name: sets served}, "worst": (ratio, what), "calls", "refused", "failed"}


def state(c):
    if c.name in _STATE:
        return _STATE[c.name]
    _lib, ops, packing = _sat()
    x, w, e = host_inputs(c)
    s = {"e": e, "w": w}
    xd = x.to(DEV)
    if c.x_planes:
        s["xs"] = ops.act_split(xd, R.IN_SLOPE)
        s["pre"] = ops.unsplit(s["xs"]).double().cpu()          # the 22 bits of pre(x) the kernel is given
        s["x"] = torch.empty_like(xd)                            # with x_split, x only gives the shape
    else:
        s["x"], s["pre"] = xd, x.double()
    wd = w.to(DEV)
    s["ksize"], s["pad_left"] = c.k, c.padding[0]
    if c.up > 1:
        wd, s["ksize"], s["pad_left"] = packing.convtranspose_as_phase_conv(wd, c.up, (c.k - c.up) // 2)
    s["wp"] = (packing.pack_conv_weight(wd, groups=c.groups, up=c.up) if c.mode == 0 else packing.pack_conv_weight_f16x3(wd, groups=c.groups, up=c.up))
    s["dev"] = {f: getattr(e, f).to(DEV) for f in e._fields}
    if c.cout % 16 == 0:
        s["res_split"] = ops.act_split(s["dev"]["res_p"], R.Y_SLOPE)
        s["y_split"] = ops.split_like(B, c.cout, c.t_out, DEV)
    else:          # (refused before anything is read or written: valid buffers of the right kind all the same)
        s["res_split"] = s["y_split"] = ops.split_like(B, 16 * (c.cout // 16 + 1), c.t_out, DEV)
    s["y"] = torch.empty(B, c.cout, c.t_out, device=DEV)
    s["sums"] = {}
    TABLE[c.name] = {"families": {}, "worst": (0.0, ""), "calls": 0, "refused": 0, "failed": 0}
    _STATE[c.name] = s
    return s


def call_kwargs(c, o, s):
    d = s["dev"]
    kw = dict(dilation=c.dil, stride=c.stride, pad_left=s["pad_left"], groups=c.groups, mode=c.mode, up=c.up, out=s["y"])
    if c.up == 1:
        kw["pad_right"] = c.padding[1]
    if o.bias:
        kw["bias"] = d["bias"]
    if o.res == "f32":
        kw["res"] = d["res"]
    elif o.res == "f32 strided":
        kw.update(res=d["res"], res_scale=R.RES_SCALE, res_toff=R.RES_TOFF, res_tstride=R.RES_TSTRIDE)
    elif o.res == "post":
        kw["post_res"] = d["res"]
    elif o.res in PLANES_RES:
        kw.update(res_split=s["res_split"], res_split_slope=R.Y_SLOPE, res_scale=R.RES_SCALE if o.res == "planes scaled" else 1.0)
    if o.act in ("relu", "relu_first"):
        kw.update(relu=True, relu_first=o.act == "relu_first")
    elif o.act == "gelu":
        kw["gelu"] = True
    if o.affine:
        kw.update(ch_scale=d["ch_scale"], ch_shift=d["ch_shift"])
    kw.update(accum=o.accum in ("accum", "accum div"), accum_div=R.ACCUM_DIV if o.accum in ("accum div", "div") else 0.0)
    if o.out != "f32":
        kw.update(y_split=s["y_split"], y_split_slope=R.Y_SLOPE, no_y=o.out == "planes")
    if o.in_lrelu:
        kw["in_lrelu"] = R.IN_SLOPE
    if c.x_planes:
        kw["x_split"] = s["xs"]
    if c.wrap:
        kw.update(x_wrap_channels=c.wrap, c_in=c.cin, t_out=c.T)
    return kw


def _worst(got, want, bound):
    """(elements outside the bound or not finite, worst |got - want| / bound) — on the device, one copy back"""
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    ratio = torch.nan_to_num(err / bound, nan=float("inf")).max()
    n, r = torch.stack([bad.sum().double(), ratio]).tolist()
    return int(n), r


def run_sets(c, sets):
    """every option set of `sets` on carrier c; returns the list of failures (strings)"""
    _lib, ops, _ = _sat()
    s = state(c)
    rec = TABLE[c.name]
    fails = []
    wants = {}
    for o in sets:
        if (o.in_lrelu,) not in s["sums"]:
            s["sums"][(o.in_lrelu,)] = pre_sum(c, s["pre"], s["w"], o.in_lrelu)
        key = R.value_key(o)
        if key not in wants:
            want, bound = R.conv(s["sums"][(o.in_lrelu,)], o, s["e"])
            wp, bp = R.planes(want, bound)
            wants[key] = tuple(t.to(DEV) for t in (want, bound, wp, bp))
        want, bound, want_p, bound_p = wants[key]
        y, ys = s["y"], s["y_split"]
        if o.accum in ("accum", "accum div") and o.out != "planes":
            y.copy_(s["dev"]["y_old"])
        else:
            y.fill_(SENTINEL if o.out == "planes" else float("nan"))
        ys.fill_(float("nan"))
        expect = refusal(c, o)
        try:
            ops.conv1d(s["x"], s["wp"], c.cout, s["ksize"], **call_kwargs(c, o, s))
        except _lib.SatError as err:
            if "(-2)" in str(err):          # SAT_ERR_HIP: the runtime failed, nothing more is started on this device
                pytest.exit(f"{c.name} [{o}]: {err}", returncode=3)
            rec["refused"] += 1
            if expect is None or expect not in str(err):
                fails.append(f"[{o}] refused with '{err}', expected {'to be served' if expect is None else repr(expect)}")
            continue
        if expect is not None:
            fails.append(f"[{o}] was served; REFUSED lists it: '{expect}'")
            continue
        full = _lib.lib().sat_last_dispatch_name().decode()
        rec["families"][full] = rec["families"].get(full, 0) + 1
        rec["calls"] += 1
        msgs = []
        if o.out == "planes":
            if not bool((y == SENTINEL).all()):
                msgs.append("no_y: the f32 buffer was written")
        else:
            n, r = _worst(y, want, bound)
            if r > rec["worst"][0]:
                rec["worst"] = (r, f"y [{o}]")
            if n:
                msgs.append(f"y: {n} elements outside the bound, worst |err| / bound {r:.3g}")
        if o.out != "f32":
            n, r = _worst(ops.unsplit(ys), want_p, bound_p)
            if r > rec["worst"][0]:
                rec["worst"] = (r, f"y_split [{o}]")
            if n:
                msgs.append(f"y_split: {n} elements outside the bound, worst |err| / bound {r:.3g}")
            if o.out == "f32 + planes" and not torch.equal(ys, ops.act_split(y, R.Y_SLOPE)):
                msgs.append("y_split != act_split(y)")
        if msgs:
            fails.append(f"[{o}] {full.split('<')[0].strip()}: " + "; ".join(msgs))
    rec["failed"] += len(fails)
    return fails


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("res", R.RES, ids=[r.replace(" ", "_") for r in R.RES])
@pytest.mark.parametrize("c", CARRIERS, ids=[c.name.replace(" ", "_") for c in CARRIERS])
def test_every_option_set(c, res):
    sets = R.lattice(f32_input=not c.x_planes, res=res)
    with _options(c.options):
        fails = run_sets(c, sets)
    torch.cuda.synchronize()
    print(f"CONVOPT {c.name} | res {res}: {len(sets)} option sets, {len(fails)} failed")
    assert not fails, f"{c.name}: {len(fails)} of {len(sets)} option sets failed:\n" + "\n".join(fails[:12])


def test_ring16_declines_e4m3_planes():
    """the one thing ring16_supports declines: SAT_SPLIT_F8 output planes (y_split_format 2), a descriptor field outside the lattice.  The call falls
    through to the 32x32x16 ring GEMM; y stays within the bound and the planes are act_split(y) in that format, bit for bit"""
    _lib, ops, _ = _sat()
    c = next(c for c in CARRIERS if c.name == "k1 ring16 gemm T 255")
    s = state(c)
    for o in R.lattice(f32_input=False, out="f32 + planes", res="f32", accum="none"):
        want, bound = (t.to(DEV) for t in R.conv(pre_sum(c, s["pre"], s["w"], False), o, s["e"]))
        served = []
        for fmt in (0, 2):
            s["y"].fill_(float("nan"))
            s["y_split"].fill_(float("nan"))
            ops.conv1d(s["x"], s["wp"], c.cout, 1, y_split_format=fmt, **call_kwargs(c, o, s))
            served.append(_lib.lib().sat_last_dispatch_name().decode().split("<")[0].strip())
            n, r = _worst(s["y"], want, bound)
            assert n == 0, (str(o), fmt, n, r)
            assert torch.equal(s["y_split"], ops.act_split(s["y"], R.Y_SLOPE, fmt=1 if fmt == 2 else 0)), (str(o), fmt)
        assert served == ["gemm_f16x3_ring16_kernel", "gemm_f16x3_ring_kernel"], (str(o), served)


def test_every_family_served_and_declined():
    """runs after the matrix (file order): every carrier reached the kernel it was meant for, and a family that carries a subset of the epilogue
    was seen both serving and declining, the declined sets served by another family within the same bound.  Prints the table."""
    problems = []
    for c in CARRIERS:
        rec = TABLE.get(c.name)
        if rec is None:
            problems.append(f"{c.name}: no case ran")
            continue
        by_family = {}
        for full, n in rec["families"].items():
            f = full.split("<")[0].strip()
            by_family[f] = by_family.get(f, 0) + n
        print(f"CONVOPT TABLE {c.name}: {rec['calls']} served, {rec['refused']} refused, {rec['failed']} failed; worst |err| / bound {rec['worst'][0]:.4f} at {rec['worst'][1]}")
        for full, n in sorted(rec["families"].items()):
            print(f"CONVOPT TABLE     {n:5d}  {full}")
        if by_family.get(c.family, 0) == 0:
            problems.append(f"{c.name}: meant to reach {c.family}, served by {sorted(by_family)}")
        if c.restricted and len(by_family) < 2:
            problems.append(f"{c.name}: {c.family} never declined an option set")
        if not c.restricted and len(by_family) > 1:
            problems.append(f"{c.name}: the options moved the call between families {sorted(by_family)}: mark the carrier restricted")
    assert not problems, "\n".join(problems)
