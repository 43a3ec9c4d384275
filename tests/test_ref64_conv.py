"""tests/ref64_conv.py pinned on the CPU, before tests/test_hip_conv_options.py holds a kernel to it:

  within the bound     the same chain evaluated in float32 torch, in the descriptor's order, stays inside the running bound for every option set of the
                       lattice at every carrier shape — a failure here means the bound formula is wrong, not a kernel;
  distinguishability   two option sets that differ in exactly one option have float64 values more than 100 bounds apart in at least 1 % of the
                       elements, or the pair is in ref64_conv.EQUIVALENT with its reason — the matrix cannot pass a kernel that ignores an option;
  the bounds table     ref64_conv gives what conv_want of tests/test_hip_bounds.py gives on the option set of every conv row of that table."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import ref64_conv as R
import test_hip_bounds as TB
import test_hip_conv_options as TC
from ref64_conv import Opt

IDS = [c.name.replace(" ", "_") for c in TC.CARRIERS]


def _sums(c, x, w, dtype):
    return {il: TC.pre_sum(c, x, w, il, dtype=dtype) for il in ((False, True) if not c.x_planes else (False,))}


@pytest.mark.parametrize("c", TC.CARRIERS, ids=IDS)
def test_float32_chain_stays_within_the_bound(c):
    x, w, e = TC.host_inputs(c)
    s64, s32 = _sums(c, x, w, torch.float64), _sums(c, x, w, torch.float32)
    worst, at, n = 0.0, None, 0
    for o in R.lattice(f32_input=not c.x_planes, out="f32"):
        want, bound = R.conv(s64[o.in_lrelu], o, e)
        got, bound32 = R.conv(s32[o.in_lrelu], o, e, dtype=torch.float32)
        assert got.dtype == torch.float32 and want.dtype == torch.float64 and torch.allclose(bound, bound32, rtol=1e-3, atol=0.0)
        assert want.shape == (TC.B, c.cout, c.t_out) and bool((bound >= R.E0 / 8).all())          # (an affine scale of 0.5 and the division by 3 shrink it at the most)
        r = float(((got.double() - want).abs() / bound).max())
        wp, bp = R.planes(want, bound)
        r = max(r, float(((F.leaky_relu(got, R.Y_SLOPE).double() - wp).abs() / bp).max()))
        if r > worst:
            worst, at = r, o
        n += 1
    print(f"REF64CONV {c.name}: {n} option sets, worst float32 |err| / bound {worst:.4f} at [{at}]")
    assert worst <= 1.0, (c.name, str(at), worst)


# five shapes, cropped to 16 channels x 96 positions of the first utterance: which options a value depends on is not a matter of the size
DISTINGUISH = ["f32 64x256 k3 dilated", "f32 up 4 k8", "f32 stride 2 k2", "f16x3 f32-in 32 rows k3", "planes k3 half-width tile"]


def _crop(c, x, w, e, C=16, T=96):
    s = {il: v[:1, :C, :T].clone() for il, v in _sums(c, x, w, torch.float64).items()}
    e = R.EpiInputs(e.bias[:C], e.ch_scale[:C], e.ch_shift[:C], e.res[:1, :C, :2 * T + 2], e.res_p[:1, :C, :T], e.y_old[:1, :C, :T])
    return s, e


@pytest.mark.parametrize("name", DISTINGUISH, ids=[n.replace(" ", "_") for n in DISTINGUISH])
def test_option_sets_that_differ_in_one_option_differ_in_value(name):
    c = next(c for c in TC.CARRIERS if c.name == name)
    sums, e = _crop(c, *TC.host_inputs(c))
    sets = R.lattice(f32_input=not c.x_planes)
    val = {o: R.conv(sums[o.in_lrelu], o, e) for o in sets if o.out == "f32"}
    pairs = same = 0
    for i, axis in enumerate(Opt._fields):
        others = [R.AXES[f] if (f != "in_lrelu" or not c.x_planes) else (False,) for f in Opt._fields if f != axis]
        values = R.AXES[axis] if (axis != "in_lrelu" or not c.x_planes) else (False,)
        for rest in itertools.product(*others):
            for va, vb in itertools.combinations(values, 2):
                a, b = Opt(*rest[:i], va, *rest[i:]), Opt(*rest[:i], vb, *rest[i:])
                pairs += 1
                reason = R.equivalent(a, b)
                (wa, ba), (wb, bb) = val[R.value_key(a)], val[R.value_key(b)]
                apart = float(((wa - wb).abs() > 100 * torch.maximum(ba, bb)).double().mean())
                if reason is not None:
                    same += 1
                    assert float((wa - wb).abs().max()) == 0.0, (str(a), str(b), reason)          # (an EQUIVALENT pair really is one)
                else:
                    assert apart >= 0.01, f"[{a}] and [{b}]: only {apart:.2%} of the elements more than 100 bounds apart"
    print(f"REF64CONV {name}: {pairs} pairs that differ in one option, {same} of them EQUIVALENT")
    assert pairs > 5000 or c.x_planes


def test_equivalent_table_is_short_and_reasoned():
    assert len(R.EQUIVALENT) <= 6 and all(len(r["reason"]) > 20 for r in R.EQUIVALENT)


def test_lattice_is_the_full_product():
    assert len(R.lattice()) == 2 * 6 * 4 * 2 * 4 * 3 * 2 and len(R.lattice(f32_input=False)) == 1152
    assert len(set(R.lattice())) == len(R.lattice())


# ---- the same answer as the bounds table -------------------------------------------------------------------------------------------------------
def test_conv_rows_are_all_recorded():
    names = {r.name for r in TB.ROWS if r.entry == "sat_conv1d_f32"}
    recorded = {name for name, _, _ in TB.CONV_ROWS}
    assert recorded <= names and len(recorded) == len(TB.CONV_ROWS) >= 35


@pytest.mark.parametrize("row", TB.CONV_ROWS, ids=[r[0].replace(" ", "_") for r in TB.CONV_ROWS])
def test_agrees_with_the_reference_of_the_bounds_table(row):
    """conv_want (what conv_case of tests/test_hip_bounds.py asserts against) and ref64_conv on the row's option set and geometry, one of its shapes"""
    name, shapes, kw = row
    Bn, T = shapes[1] if len(shapes) > 1 else shapes[0]
    cin, cout, k = kw["cin"], kw["cout"], kw["k"]
    dil, stride, groups, wrap = kw.get("dil", 1), kw.get("stride", 1), kw.get("groups", 1), kw.get("wrap", 0)
    halo = dil * (k - 1)
    pl, pr = kw.get("pads") or (halo // 2, halo - halo // 2)
    T_q = T if wrap else (T + pl + pr - halo - 1) // stride + 1
    assert T_q > 0
    slope = kw.get("slope")
    x = TB.rand(Bn, wrap or cin, T, seed=T + cin)
    w = TB.rand(cout, cin // groups, k, seed=2, scale=(cin // groups * k) ** -0.5)
    b, sc, sh, acc0 = TB.rand(cout, seed=3), TB.rand(cout, seed=9).abs() + 0.5, TB.rand(cout, seed=10), TB.rand(Bn, cout, T_q + kw.get("ypitch", 0), seed=5)
    res, toff, tstride, scale = kw.get("res"), kw.get("res_toff", 0), kw.get("res_tstride", 1), kw.get("res_scale", 1.0)
    r = None if res is None else TB.rand(Bn, cout, (T_q - 1) * tstride + toff + 1 if res == "f32" else T_q, seed=4)
    opts = {f: kw.get(f, False) for f in ("post_res", "accum", "affine", "relu", "gelu", "relu_first")}
    pre = TB._lrelu(x.double(), slope)          # (a row on planes: the kernel is given 22 bits of this; the two references take the same tensor)
    theirs = TB.conv_want(pre, w, b, r, sc, sh, acc0, T_q, cin=cin, dil=dil, stride=stride, pads=(pl, pr), groups=groups, res_toff=toff, res_tstride=tstride,
                          res_scale=scale, accum_div=kw.get("accum_div", 0.0), wrap=wrap, **opts)
    s = R.pre_sum(x, w, dilation=dil, stride=stride, pads=(pl, pr), groups=groups, in_slope=slope, wrap=wrap, t_q=T_q)
    ours, bound = R.epilogue(s, bias=b, res=r, res_scale=scale, res_toff=toff, res_tstride=tstride, res_after=opts["post_res"], res_planes=res == "planes",
                             ch_scale=sc if opts["affine"] else None, ch_shift=sh if opts["affine"] else None, relu=opts["relu"], relu_first=opts["relu_first"],
                             gelu=opts["gelu"], y_old=acc0 if opts["accum"] else None, accum_div=kw.get("accum_div", 0.0) if opts["accum"] else 0.0)
    assert ours.shape == theirs.shape == (Bn, cout, T_q)
    d = float((ours - theirs).abs().max())
    assert d <= 1e-12 * max(1.0, float(theirs.abs().max())), (name, d)
    assert bool(torch.isfinite(bound).all()) and bool((bound >= R.E0 / 8).all())
