"""sat_generator_input_f32 (include/satools_hip_geninput.h; csrc/geninput/generator_input.hip) on the GPU.

* With S = 1, slice_stat = NULL and a contiguous bn the launch equals sat_f0_stats_f32 -> sat_f0_apply_f32 -> sat_assemble_input_f32 BIT FOR BIT,
  in x and in f0_norm: the kernel restates those kernels' statements, and this test is what holds the two sources together.
* Per-slice statistics against float64 at the derived bound 3 * 2^-24 * |q| (tests/ref64_geninput.py: two correctly rounded operations);
  the gather, the copies, the quantiser and the noise on the kernel's own normalised values: equality.
* A strided bn (the permuted [B, T, C] view, a padded row pitch) equals the contiguous call bit for bit, on both sides of the 64 x 64 tile.
* Red zones (tests/moat.py) around every buffer through the C entry point, NULL f0_norm, NULL spk and an out-of-range slice_stat entry
  included: the slice is skipped, nothing outside is written.
* Refusals carry their message and launch nothing.

Largest observed error / bound: printed, and written to the file SAT_GENINPUT_RATIOS names (profiles/geninput_error_ratios.txt).
Needs a real MI355X: run with `-m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ref64_geninput as r64
from moat import Buf, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 64
# both sides of the existing kernels' 256-column block, T_f0 - T in {0, 1} as the tags have it, both resampling directions
TIMES = [(1, 1), (7, 9), (63, 64), (255, 256), (256, 256), (257, 258), (513, 250), (250, 513)]
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    yield
    lines = [f"{k:28s} {r:8.4f}   at {case}" for k, (r, case) in sorted(_RATIOS.items())]
    print("\nlargest observed error / derived bound:\n" + "\n".join(lines))
    path = os.environ.get("SAT_GENINPUT_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_hip_geninput.py: largest observed error / derived bound (a ratio above 1 fails)\n")
            f.write("\n".join(lines) + "\n")


def _sat():
    import satools_amd  # noqa: F401
    from satools_amd import _lib, ops
    return _lib, ops


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _track(B, n, g, voiced=0.6):
    f0 = 80.0 + 220.0 * torch.rand(B, n, generator=g)
    return torch.where(torch.rand(B, n, generator=g) < voiced, f0, torch.zeros(B, n))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _three_calls(bn, f0, quant, noise, spk):
    """the existing sequence on contiguous tensors -> (x, f0_norm)"""
    _lib, ops = _sat()
    l, ptr, st = _lib.lib(), _lib.ptr, _lib.stream
    n = f0.numel()
    stats = torch.empty(2, dtype=torch.float32, device=DEV)
    _lib.check(l.sat_f0_stats_f32(ptr(f0), n, ptr(stats), st()), "sat_f0_stats_f32")
    norm, tr = f0.clone(), f0.clone()
    _lib.check(l.sat_f0_apply_f32(ptr(norm), n, ptr(stats), 0, None, st()), "sat_f0_apply_f32")
    _lib.check(l.sat_f0_apply_f32(ptr(tr), n, ptr(stats), int(quant), ptr(noise), st()), "sat_f0_apply_f32")
    B = bn.shape[0]
    x = ops.assemble_input(bn, tr.reshape(B, -1), spk, 0 if spk is None else spk.shape[1])
    return x, norm, stats


@pytest.mark.parametrize("T,T_f0", TIMES, ids=lambda v: str(v))
def test_equals_the_existing_three_calls_bit_for_bit(T, T_f0):
    _lib, ops = _sat()
    g = _gen(1, T, T_f0)
    bn_all = torch.randn(3, 256, T, generator=g).to(DEV)
    spk_all = torch.rand(3, 5, generator=g).to(DEV)
    f0_all = _track(3, T_f0, g)
    f0_all[0, 0] = 117.0                                   # (a voiced frame in every length, T_f0 = 1 included)
    noise_all = torch.randn(3, T_f0, generator=g).to(DEV)
    n = 0
    for B in (1, 3):
        f0 = f0_all[:B].clone()
        if B == 3:
            f0[1] = 0.0                                    # a row that is all zeros
            f0[2] = 0.0
            f0[2, T_f0 // 2] = 203.0                       # a row with one voiced frame
        f0 = f0.unsqueeze(0).contiguous().to(DEV)          # [1, B, T_f0]
        for n_spk in (0, 1, 5):
            spk = spk_all[:B, :n_spk].contiguous() if n_spk else None
            for c_bn in (1, 33, 256):
                bn = bn_all[:B, :c_bn].contiguous()
                for quant in (0, 16):
                    for noise in (None, noise_all[:B].contiguous()):
                        want_x, want_norm, stats = _three_calls(bn, f0, quant, noise, spk)
                        keep = f0.clone()
                        x, norm = ops.generator_input(bn, f0, stats.view(1, 2), None, quant, noise, spk)
                        case = (B, n_spk, c_bn, quant, noise is not None)
                        assert _same_bits(x, want_x), case
                        assert _same_bits(norm, want_norm), case
                        assert _same_bits(f0, keep), case                      # the raw track is not written
                        x2, norm2 = ops.generator_input(bn, f0, stats.view(1, 2), None, quant, noise, spk)
                        assert _same_bits(x2, x) and _same_bits(norm2, norm), case          # twice for the same bits
                        n += 1
    assert n == 2 * 3 * 3 * 2 * 2
    _RATIOS.setdefault("x, f0_norm (S = 1, NULL)", (0.0, "bit for bit equal to f0_stats -> f0_apply -> assemble_input in every case"))


def test_one_voiced_frame_in_the_batch_gives_the_nan_of_the_existing_calls():
    _lib, ops = _sat()
    f0 = torch.zeros(1, 1, 40)
    f0[0, 0, 7] = 150.0
    f0 = f0.to(DEV)
    bn = torch.randn(1, 3, 39, generator=_gen(2)).to(DEV)
    want_x, want_norm, stats = _three_calls(bn, f0, 0, None, None)
    x, norm = ops.generator_input(bn, f0, stats.view(1, 2))
    assert bool(torch.isnan(stats[1])) and int(torch.isnan(norm).sum()) == 1
    assert _same_bits(x, want_x) and _same_bits(norm, want_norm)
    zeros = torch.zeros(1, 1, 40, device=DEV)
    x, norm = ops.generator_input(bn, zeros, stats.view(1, 2))                  # all unvoiced: every zero stays zero, NaN statistics or not
    assert not norm.any() and not x[:, 3].any() and _same_bits(x[:, :3], bn)


@pytest.mark.parametrize("S,R", [(3, 1), (1, 3), (2, 2), (5, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("T,T_f0", [(63, 64), (257, 258), (250, 513)], ids=lambda v: str(v))
def test_per_slice_statistics_against_float64(S, R, T, T_f0):
    _lib, ops = _sat()
    B, n_stats, c_bn, n_spk = S * R, 4, 33, 5
    g = _gen(3, S, R, T, T_f0)
    bn = torch.randn(B, c_bn, T, generator=g)
    spk = torch.rand(B, n_spk, generator=g)
    f0 = _track(B, T_f0, g).reshape(S, R, T_f0)
    f0[0, 0] = 0.0                                                              # an all-zero row among voiced ones
    stats = torch.stack([100.0 + 100.0 * torch.rand(n_stats, generator=g), 10.0 + 40.0 * torch.rand(n_stats, generator=g)], dim=1)
    table = {1: [2], 3: [3, 0, 3], 2: [1, 1], 5: [3, 1, 0, 1, 2]}[S]              # repeated and permuted entries
    noise = torch.randn(B, T_f0, generator=g)
    want_x, want_norm = r64.generator_input(bn.numpy(), f0.numpy(), stats.numpy(), table, spk.numpy())
    idx = r64.interp_index(T, T_f0)
    for quant, nz in ((0, None), (16, None), (64, noise), (0, noise)):
        x, norm = ops.generator_input(bn.to(DEV), f0.to(DEV), stats.to(DEV), table, quant, None if nz is None else nz.to(DEV), spk.to(DEV))
        x, norm = x.cpu(), norm.cpu()
        err = (norm.double().numpy() - want_norm)
        bound = r64.NORM_BOUND * np.abs(want_norm)
        assert not norm[f0 == 0].any() and np.all(np.abs(err) <= bound), (quant, float(np.abs(err).max()))
        ratio = float(np.max(np.abs(err)[bound > 0] / bound[bound > 0]))
        case = f"S{S} R{R} T{T} T_f0 {T_f0}"
        if ratio > _RATIOS.get("f0_norm (per slice)", (-1.0, ""))[0]:
            _RATIOS["f0_norm (per slice)"] = (ratio, case)
        # everything else is a copy, a gather, or torch's own float32 quantiser / sum on the kernel's normalised values
        assert _same_bits(x[:, :c_bn], bn) and _same_bits(x[:, c_bn + 1:], spk[:, :, None].expand(B, n_spk, T).contiguous())
        flat = norm.reshape(B, T_f0).numpy()
        tr = r64.transform32(flat, quant, None if nz is None else nz.numpy())
        assert np.array_equal(x[:, c_bn].numpy().view(np.int32), tr[:, idx].view(np.int32)), (case, quant)
        if quant == 0 and nz is None:
            assert np.all(np.abs(x[:, c_bn].double().numpy() - want_x[:, c_bn]) <= r64.NORM_BOUND * np.abs(want_x[:, c_bn]))
    _RATIOS.setdefault("bn, F0 gather, spk rows", (0.0, "bit for bit equal to the copy / gather / float32 quantiser and sum in every case"))


@pytest.mark.parametrize("c_bn", (1, 63, 64, 65, 130), ids=lambda v: f"C{v}")
def test_a_strided_bn_equals_the_contiguous_call(c_bn):
    _lib, ops = _sat()
    for T in (1, 63, 64, 65, 200):
        g = _gen(4, c_bn, T)
        B, T_f0 = 3, T + 1
        btc = torch.randn(B, T, c_bn, generator=g).to(DEV)                      # what extract_bn writes
        f0 = _track(B, T_f0, g).unsqueeze(0).to(DEV)
        stats = torch.tensor([[150.0, 30.0]], device=DEV)
        spk = torch.rand(B, 2, generator=g).to(DEV)
        view = btc.permute(0, 2, 1)
        assert c_bn == 1 or T == 1 or not view.is_contiguous()
        want, wn = ops.generator_input(view.contiguous(), f0, stats, None, 0, None, spk)
        got, gn = ops.generator_input(view, f0, stats, None, 0, None, spk)
        assert _same_bits(got, want) and _same_bits(gn, wn), T
        assert _same_bits(got[:, :c_bn], view.contiguous())
        padded = torch.full((B, c_bn + 2, T + 3), float("nan"), device=DEV)    # a row pitch and a channel pitch, time axis contiguous
        padded[:, 1:1 + c_bn, 2:2 + T] = view
        got, _ = ops.generator_input(padded[:, 1:1 + c_bn, 2:2 + T], f0, stats, None, 0, None, spk, want_norm=False)
        assert _same_bits(got, want), T


# ---- red zones ------------------------------------------------------------------------------------------------------------------------
def _moat_case(B, S, c_bn, T, T_f0, n_spk, table, with_norm=True, with_noise=True, permuted=False, n_stats=3, quant=16):
    _lib, _ = _sat()
    R = B // S
    g = _gen(5, B, S, c_bn, T, T_f0, n_spk)
    bn = torch.randn(B, T, c_bn, generator=g) if permuted else torch.randn(B, c_bn, T, generator=g)
    f0 = _track(B, T_f0, g).reshape(S, R, T_f0)
    stats = torch.stack([100.0 + 100.0 * torch.rand(n_stats, generator=g), 10.0 + 40.0 * torch.rand(n_stats, generator=g)], dim=1)
    C_all = c_bn + 1 + n_spk
    skipped = torch.zeros(B, dtype=torch.bool)
    if table is not None:
        skipped = torch.tensor([not 0 <= k < n_stats for k in table]).repeat_interleave(R)
    x_keep = torch.zeros(B, C_all, T, dtype=torch.bool)
    x_keep[skipped, c_bn] = True                                                # the F0 rows of a skipped slice are not written
    specs = [Buf("bn", "in", tuple(bn.shape), data=bn), Buf("f0", "in", (S, R, T_f0), data=f0), Buf("stats", "in", (n_stats, 2), data=stats),
             Buf("x", "out", (B, C_all, T), untouched=x_keep)]
    if table is not None:
        specs.append(Buf("slice_stat", "in", (S,), torch.int32, data=torch.tensor(table, dtype=torch.int32), index=True))
    if with_noise:
        specs.append(Buf("noise", "in", (B, T_f0), data=torch.randn(B, T_f0, generator=g)))
    if n_spk:
        specs.append(Buf("spk", "in", (B, n_spk), data=torch.rand(B, n_spk, generator=g)))
    if with_norm:
        specs.append(Buf("f0_norm", "out", (S, R, T_f0), untouched=skipped.reshape(S, R, 1).expand(S, R, T_f0).contiguous()))

    def call(t):
        P = lambda k: t[k].data_ptr() if k in t else None           # noqa: E731
        sb, sc, st = (T * c_bn, 1, c_bn) if permuted else (c_bn * T, T, 1)
        d = _lib.GenInputDesc(B=B, C_bn=c_bn, T=T, T_f0=T_f0, S=S, R=R, n_stats=n_stats, n_spk=n_spk, quant_bins=quant, reserved=0,
                              bn_bstride=sb, bn_cstride=sc, bn_tstride=st, bn=P("bn"), f0=P("f0"), stats=P("stats"), slice_stat=P("slice_stat"),
                              noise=P("noise"), spk=P("spk"), x=P("x"), f0_norm=P("f0_norm"))
        _lib.check(_lib.lib().sat_generator_input_f32(C.byref(d), _lib.stream()), "sat_generator_input_f32")

    return specs, call


@pytest.mark.parametrize("case", [
    dict(B=1, S=1, c_bn=1, T=1, T_f0=1, n_spk=0, table=None),
    dict(B=3, S=3, c_bn=65, T=63, T_f0=64, n_spk=5, table=[2, 0, 2]),
    dict(B=3, S=1, c_bn=64, T=257, T_f0=258, n_spk=1, table=[1], with_norm=False),                  # NULL f0_norm
    dict(B=3, S=3, c_bn=33, T=65, T_f0=66, n_spk=0, table=[0, 1, 2], permuted=True),                # NULL spk, the LDS tile
    dict(B=2, S=1, c_bn=130, T=64, T_f0=513, n_spk=3, table=None, permuted=True, with_noise=False),
    dict(B=3, S=3, c_bn=33, T=129, T_f0=130, n_spk=2, table=[1, 3, 0]),                             # entry 3 of 0 .. 2: slice 1 is skipped
    dict(B=4, S=2, c_bn=5, T=250, T_f0=513, n_spk=2, table=[-1, 2], permuted=True),                 # a negative entry: rows 0 and 1 skipped
], ids=lambda c: "B{B}S{S}C{c_bn}T{T}F{T_f0}N{n_spk}".format(**c) + ("p" if c.get("permuted") else "") + str(c["table"]).replace(" ", ""))
def test_red_zones_around_every_buffer(case):
    specs, call = _moat_case(**case)
    v, moat, plain = run_case(specs, call, device=DEV, sync=torch.cuda.synchronize)
    assert not v, "\n".join(str(e) for e in v)
    # and the owned outputs are the right ones: bn rows copied, in whichever layout they came
    bn = next(s for s in specs if s.name == "bn").data
    bn = bn.permute(0, 2, 1) if case.get("permuted") else bn
    assert _same_bits(moat.t["x"][:, :case["c_bn"]], bn.contiguous())


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_their_message_and_launch_nothing():
    _lib, ops = _sat()
    B, c_bn, T, T_f0 = 2, 3, 10, 11
    bn = torch.randn(B, c_bn, T, generator=_gen(6)).to(DEV)
    f0 = _track(B, T_f0, _gen(7)).unsqueeze(0).to(DEV)
    stats = torch.tensor([[150.0, 30.0], [120.0, 20.0]], device=DEV)
    x = torch.full((B, c_bn + 1, T), 7.0, device=DEV)
    norm = torch.full((1, B, T_f0), 7.0, device=DEV)

    def desc(**kw):
        a = dict(B=B, C_bn=c_bn, T=T, T_f0=T_f0, S=1, R=B, n_stats=2, n_spk=0, quant_bins=0, reserved=0, bn_bstride=c_bn * T, bn_cstride=T,
                 bn_tstride=1, bn=bn.data_ptr(), f0=f0.data_ptr(), stats=stats.data_ptr(), slice_stat=None, noise=None, spk=None,
                 x=x.data_ptr(), f0_norm=norm.data_ptr())
        a.update(kw)
        return _lib.GenInputDesc(**a)

    def refused(d, message):
        assert _lib.lib().sat_generator_input_f32(None if d is None else C.byref(d), _lib.stream()) == -1
        assert message in _lib.lib().sat_last_error().decode(), _lib.lib().sat_last_error()

    refused(None, "generator_input: null descriptor")
    for k in ("bn", "f0", "stats", "x"):
        refused(desc(**{k: None}), "generator_input: null pointer")
    refused(desc(n_spk=2), "generator_input: spk and n_spk = 2 disagree")
    refused(desc(spk=stats.data_ptr()), "generator_input: spk and n_spk = 0 disagree")
    for k in ("B", "C_bn", "T", "T_f0", "S", "R", "n_stats"):
        refused(desc(**{k: 0}), "generator_input: bad sizes")
    refused(desc(quant_bins=-1), "generator_input: bad sizes")
    refused(desc(S=2, R=2), "generator_input: S * R = 2 * 2 is not B = 2")
    refused(desc(B=65536, R=65536), "generator_input: batch of 65536 utterances exceeds the 65535 one launch takes")
    refused(desc(C_bn=65535), "generator_input: 65536 channels exceed the 65535 one launch takes")
    for strides in ((0, T, 1), (c_bn * T, 0, 1), (c_bn * T, T, 0), (-c_bn * T, T, 1), (c_bn * T, T - 1, 1), (c_bn * T - 1, T, 1), (T, T, 1),
                    (c_bn * T, 1, c_bn - 1)):
        refused(desc(bn_bstride=strides[0], bn_cstride=strides[1], bn_tstride=strides[2]), "let elements alias")
    # the table is the wrapper's: an entry outside it is refused on the host, by name
    with pytest.raises(_lib.SatError, match=r"generator_input: slice_stat\[1\] = 2 outside 0 \.\. 1"):
        ops.generator_input(bn, f0.reshape(2, 1, T_f0), stats, [0, 2])
    with pytest.raises(_lib.SatError, match=r"generator_input: slice_stat\[0\] = -1 outside 0 \.\. 1"):
        ops.generator_input(bn, f0, stats, [-1])
    with pytest.raises(_lib.SatError, match="slice_stat has 2 entries for 1 slices"):
        ops.generator_input(bn, f0, stats, [0, 1])
    with pytest.raises(_lib.SatError, match="S \\* R = 1 \\* 2 is not B = 3"):
        ops.generator_input(torch.zeros(3, c_bn, T, device=DEV), f0, stats)
    with pytest.raises(_lib.SatError, match="let elements alias"):
        ops.generator_input(bn[:1].expand(B, c_bn, T), f0, stats)
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((norm == 7.0).all())                  # nothing was launched
    # and a valid call still runs and is right (no sticky error)
    got, gn = ops.generator_input(bn, f0, stats, [1])
    want, wn = r64.generator_input(bn.cpu().numpy(), f0.cpu().numpy(), stats.cpu().numpy(), [1])
    assert np.all(np.abs(gn.cpu().double().numpy() - wn) <= r64.NORM_BOUND * np.abs(wn)) and _same_bits(got[:, :c_bn], bn)
