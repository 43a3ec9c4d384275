"""No kernel writes or reads outside its buffers: every entry point of include/satools_hip.h that launches a kernel, called through the
C ABI with EVERY buffer of the call carved out of a red-zoned allocation (tests/moat.py; proven on the CPU by tests/test_moat_host.py),
under two fills of everything the call does not own as an input:
    W    a guard zone or a region the call was told not to write changed
    R/U  the owned outputs under fill A (0xFF: NaN) and fill B (0x47: large finite) differ in a bit
    E    the owned outputs differ from the same call on plainly allocated tensors, bit for bit
and, for the single-kernel rows, against a float64 restatement at that kernel's existing bound (quoted from its existing test — the
edge shapes here are new).  The table is ROWS: one row per (entry point, arithmetic / layout / option), its shapes taken from the tile
constants of the kernel in csrc/ — the time axis at 1, tile - 1, tile, tile + 1 and an odd multi-tile length, B = 1 and an odd B > 1, so that
the ragged tile is in the last row of the last batch, the one place no value test can see.  Every call is a valid call on valid
memory: the zones are part of one legal allocation, nothing here passes a short buffer.  Conv rows name the kernel family they mean to
hit (sat_last_dispatch_name); FAMILIES, every dispatch-name string of csrc/, must have been seen when the file is done.
tests/test_moat_host.py::test_every_entry_point_has_a_bounds_row_or_launches_no_kernel imports ROWS / EXEMPT without touching a GPU.
Needs a real MI355X: run with `-m gpu`."""
import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref64
import ref64_asv
import ref64_resnet
from moat import Buf, run_case
from ref64 import U

DEV = "cuda"
ULP = 2.0 * U
F16, U8, I16, I32, I64 = torch.float16, torch.uint8, torch.int16, torch.int32, torch.int64

# Every SAT_LAUNCH_CHECK("...") string of csrc/ (tests/test_moat_host.py holds this list against the sources).  FAMILIES: the names an entry point
# leaves as its LAST launch, what sat_last_dispatch_name() shows after a call — each must have been seen when the table is done; the conv-shaped
# rows also assert the one they meant to hit.  INNER: launches inside a multi-launch entry point, covered by that entry point's rows.
FAMILIES = [
    "conv1d_mfma_kernel", "conv1d_f16x3_kernel", "conv1d_f16x3_k1_kernel", "conv1d_f16x3_planes_lean_kernel",
    "conv1d_f16x3_ring16_kernel", "conv1d_f16x3_ring16_kernel (F8: 8-bit cross terms)",
    "gemm_f16x3_ring16_kernel", "gemm_f16x3_ring_kernel", "gemm_f16x3_walk16_kernel",
    "resblock_pair_f16x3_kernel", "resblock_pair16_kernel", "resblock_pair32_kernel", "resblock_pair64_kernel", "pair32s_kernel", "pairw_kernel",
    "mrf16_kernel", "ups2_kernel", "conv2d_mfma_kernel", "conv2d_stem_kernel",
    "act_split_kernel", "planes_f8_sidecar_kernel", "convpost_kernel", "cmvn_pad_kernel", "pad_replicate_kernel", "vq_kernel", "vq_tiled_kernel",
    "f0_stats_kernel", "f0_apply_kernel", "f0_mean_reversion_kernel", "assemble_kernel", "tdnnf_unfold15_kernel", "log_softmax_channels_kernel",
    "pcm16_from_f32_kernel", "pcm16_to_f32_kernel", "yaapt_refine_dp_kernel", "w2v2_conv0_kernel", "layernorm_ch_kernel", "layernorm_ch_kernel<conv0>",
    "softmax_cols_kernel", "transpose_heads_kernel", "attention_f16x3_kernel", "melspec_logmel_kernel", "instnorm_rows_kernel", "row_mean_rows_kernel",
    "add3_kernel", "se_gate_add_kernel", "tanh_kernel", "attentive_stats_kernel", "l2norm_rows_kernel", "res2_chain_kernel", "linear_rows_kernel",
    "cohort_topk_stats_kernel", "trial_scores_kernel", "segment_mean_l2norm_kernel", "se_scale_add_relu_kernel", "row_mean_std_kernel",
]
INNER = {"fbank_frames_kernel": "sat_fbank_cmvn_pad_f32", "row_mean_kernel": "sat_fbank_cmvn_pad_f32", "mrf_pack_kernel": "sat_resblock_mrf_f16x3",
         "planes_range_kernel": "sat_hifigan_forward_f32"}
INNER.update({"yaapt_%s_kernel" % n: "sat_yaapt_f32" for n in ("prefilter", "stage_twiddles", "nlfer", "energy_norm", "spec", "spec_peaks", "spec_post",
                                                                "frame_means", "nccf")})
SEEN = set()

EXEMPT = {n: "launches no kernel" for n in (
    "sat_abi_version", "sat_last_error", "sat_last_dispatch_name", "sat_device_info",
    "sat_mrf_debug_stamps", "sat_attention_debug_stamps", "sat_pair32_debug_stamps", "sat_convring_debug_stamps",
    "sat_conv1d_f8r_supported", "sat_upsample_grouped_supported", "sat_convtranspose_zero_taps", "sat_resblock_mrf_supported",
    "sat_resblock_mrf_scratch_bytes", "sat_upsample2_supported", "sat_conv_set_option", "sat_conv1d_packed_dims", "sat_convtranspose_phase_dims",
    "sat_hifigan_create", "sat_hifigan_num_convs", "sat_hifigan_set_conv", "sat_hifigan_set_conv_descale", "sat_hifigan_set_conv_f8r",
    "sat_hifigan_workspace_bytes", "sat_hifigan_destroy", "sat_hifigan_set_option", "sat_hifigan_get_option", "sat_hifigan_set_range_probe",
    "sat_fbank_workspace_bytes", "sat_yaapt_workspace_bytes")}
EXEMPT["sat_clock_probe"] = "diagnostic: one wave samples two clock counters for tools/clock_probe.py while other streams work; not on any product path"


# ---- the table's machinery -----------------------------------------------------------------------------------------------------
@dataclass
class Case:
    specs: list = field(default_factory=list)
    call: object = None          # call(tensors by name)
    ref: object = None           # ref(tensors of the fill-A run): float64 assertions
    family: str = None
    options: tuple = ()          # (name, value, default) of sat_conv_set_option for the duration of the case
    tol: float = None            # entry points with floating-point atomics only (none)
    data: dict = field(default_factory=dict)          # the generated inputs by name (tests/test_hip_tile_walk.py cuts sub-batches and crops out of them)

    def _add(self, name, role, shape=None, dtype=torch.float32, data=None, **kw):
        if data is not None:
            data = data.detach().cpu().contiguous()
            shape, dtype = tuple(data.shape), data.dtype
        self.specs.append(Buf(name, role, tuple(shape), dtype, data=data, **kw))

    def inp(self, name, data, **kw):
        self._add(name, "in", data=data, **kw)

    def inout(self, name, data, **kw):
        self._add(name, "inout", data=data, **kw)

    def out(self, name, shape, dtype=torch.float32, **kw):
        self._add(name, "out", shape, dtype, **kw)

    def ws(self, name, nbytes):
        self._add(name, "workspace", (int(nbytes),), U8)

    def untouched(self, name, shape, dtype=torch.float32):
        self._add(name, "untouched", shape, dtype)


@dataclass
class Row:
    entry: str                   # the C-ABI function
    name: str
    shapes: list
    make: object                 # make(*shape) -> Case (runs on the GPU box only)


ROWS = []


def row(entry, name, shapes):
    def deco(fn):
        ROWS.append(Row(entry, name, [s if isinstance(s, tuple) else (s,) for s in shapes], fn))
        return fn
    return deco


def _sat():
    import satools_amd  # noqa: F401
    from satools_amd import _lib, ops, packing
    return _lib, ops, packing


def _L():
    return _sat()[0].lib()


def _ok(status, what):
    _sat()[0].check(status, what)


def _stream():
    return _sat()[0].stream()


def P(t):
    return None if t is None else t.data_ptr()


def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def mask_of(shape, *index):
    m = torch.zeros(shape, dtype=torch.bool)
    m[index] = True
    return m


def times(tile, lo=1):
    """the time axis of a kernel with `tile` positions per block: 1, tile - 1, tile, tile + 1 and an odd multi-tile length, B = 1 and an odd
    B > 1 (the multi-tile length among them) — the ragged tile sits in the last row of the last batch in all of them"""
    ts = sorted({max(lo, 1), max(lo, tile - 1), max(lo, tile), tile + 1, 2 * tile + 37})
    return [((3 if i % 2 or i == len(ts) - 1 else 1), t) for i, t in enumerate(ts)]


def maxerr(got, want):
    return float((got.detach().cpu().double() - want.double()).abs().max())


def bounded(kernel, got, want, bound):
    """|got - want| <= bound elementwise (a bound of 0 demands equality); prints the figure before it asserts"""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (kernel, got.shape, want.shape)
    err = (got - want).abs()
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    worst = float((err - b).max()) if err.numel() else 0.0
    print(f"{kernel}: max error {float(err.max()) if err.numel() else 0.0:.3e}, worst error - bound {worst:.3e}")
    assert bool(torch.isfinite(got).all()) and worst <= 0.0, (kernel, float(err.max()), worst)


class _options:
    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        for n, v, _ in self.opts:
            _ok(_L().sat_conv_set_option(n.encode(), v), "sat_conv_set_option")

    def __exit__(self, *a):
        for n, _, d in self.opts:
            _ok(_L().sat_conv_set_option(n.encode(), d), "sat_conv_set_option")


def _id(p):
    r, s = p
    return f"{r.entry[4:]}:{r.name}-" + "x".join(str(v) for v in s)


# ---- sample formats, padding, framing of the bottleneck net (csrc/bottleneck.hip, fbank.hip) --------------------------------
@row("sat_pcm16_to_f32", "all", [1, 255, 256, 257, 4099])
def _(n):
    c = Case()
    x = torch.randint(-32768, 32768, (n,), generator=torch.Generator().manual_seed(n)).to(I16)
    c.inp("x", x)
    c.out("y", (n,))
    c.call = lambda t: _ok(_L().sat_pcm16_to_f32(P(t["x"]), P(t["y"]), n, _stream()), "sat_pcm16_to_f32")
    c.ref = lambda t: bounded("pcm16_to_f32", t["y"], x.double() / 32768, 0)
    return c


@row("sat_pcm16_from_f32", "all", [1, 255, 256, 257, 4099])
def _(n):
    c = Case()
    x = rand(n, seed=n, scale=0.6)
    c.inp("x", x)
    c.out("y", (n,), I16)
    c.call = lambda t: _ok(_L().sat_pcm16_from_f32(P(t["x"]), P(t["y"]), n, _stream()), "sat_pcm16_from_f32")
    c.ref = lambda t: bounded("pcm16_from_f32", t["y"], torch.from_numpy(np.clip(np.rint(x.double().numpy() * 32768), -32768, 32767)), 0)
    return c


@row("sat_pad_replicate_f32", "all", [(1, 1, 1, 4, 4, 0), (3, 5, 255, 19, 19, 1), (3, 2, 256, 0, 4, 0), (1, 3, 257, 19, 0, 1), (3, 3, 549, 4, 19, 1)])
def _(B, ch, T, left, right, inter):
    c = Case()
    x = rand(B, ch, T, seed=T)
    c.inp("x", x)
    c.out("y", (B, ch, left + T + right))
    c.call = lambda t: _ok(_L().sat_pad_replicate_f32(P(t["x"]), P(t["y"]), B, ch, T, left, right, inter, _stream()), "sat_pad_replicate_f32")
    c.ref = lambda t: bounded("pad_replicate", t["y"], ref64.pad_replicate(x, left, right, bool(inter)), 0)
    return c


@row("sat_tdnnf_unfold15_f32", "all", [(1, 4, 1), (3, 6, 7), (3, 16, 40), (1, 6, 255), (3, 4, 257)])       # (D even: the entry refuses odd feature counts)
def _(B, D, T):
    c = Case()
    x = rand(B, D, T, seed=T)
    tq = (2 * (T - 1)) // 3 + 1
    c.inp("x", x)
    c.out("win", (B, D, tq))
    c.out("byp", (B, D, tq))
    c.call = lambda t: _ok(_L().sat_tdnnf_unfold15_f32(P(t["x"]), P(t["win"]), P(t["byp"]), B, D, T, _stream()), "sat_tdnnf_unfold15_f32")

    def ref(t):
        rw, rb = ref64.tdnnf_unfold15(x)
        bounded("tdnnf_unfold15 win", t["win"], rw, 0)
        bounded("tdnnf_unfold15 byp", t["byp"], rb, 0)
    c.ref = ref
    return c


@row("sat_log_softmax_channels_f32", "all", [(1, 1, 1), (3, 5, 15), (1, 16, 16), (3, 17, 17), (3, 3280, 37)])
def _(B, Cn, T):
    c = Case()
    x = rand(B, Cn, T, seed=Cn + T, scale=4.0)
    c.inout("x", x)
    c.call = lambda t: _ok(_L().sat_log_softmax_channels_f32(P(t["x"]), B, Cn, T, _stream()), "sat_log_softmax_channels_f32")

    def ref(t):          # the bound of tests/test_hip_small_kernels.py::test_log_softmax_channels
        want, a = ref64.log_softmax_channels(x)
        groups = math.ceil(Cn / 16)
        dlse = (Cn / 16 + 24) * U * a["lse"].abs().clamp(min=1.0) + U * (a["E"] + 1 * 2 * (groups + 2)) + 2 * ULP * a["logtot"].abs()
        bounded("log_softmax_channels", t["x"], want, dlse + U * want.abs())
    c.ref = ref
    return c


def _fbank_tables():
    from satools_amd import asrbn
    mel = asrbn.mel_banks(80)
    nz = mel > 0
    lo = torch.where(nz.any(1), nz.float().argmax(1), torch.zeros(80, dtype=torch.long))
    hi = torch.where(nz.any(1), mel.shape[1] - torch.flip(nz, [1]).float().argmax(1), torch.zeros(80, dtype=torch.long))
    return asrbn.povey_window(), mel, lo.to(I32), hi.to(I32)


@row("sat_fbank_cmvn_pad_f32", "cmvn+pad19", [(1, 480), (3, 640), (1, 800), (3, 2011), (3, 8000)])
def _(B, n):
    from satools_amd import synthetic
    c = Case()
    wav = synthetic.rand_batch(n, B, n) * 32768
    win, mel, lo, hi = _fbank_tables()
    m, pad = (n + 80) // 160, 19
    nws = _L().sat_fbank_workspace_bytes(B, n)
    c.inp("wav", wav)
    c.inp("window", win)
    c.inp("mel", mel)
    c.inp("mel_lo", lo, index=True)
    c.inp("mel_hi", hi, index=True)
    c.ws("ws", nws)
    c.out("feats", (B, 80, m + 2 * pad))
    c.call = lambda t: _ok(_L().sat_fbank_cmvn_pad_f32(P(t["wav"]), P(t["feats"]), P(t["window"]), P(t["mel"]), P(t["mel_lo"]), P(t["mel_hi"]), P(t["ws"]), nws,
                                                      B, n, 1.0, 80, pad, 1, _stream()), "sat_fbank_cmvn_pad_f32")

    def ref(t):          # tests/test_hip_parity.py::test_fbank_cmvn_pad_matches_oracle: 3e-4 against the CPU oracle
        from oracle import fbank as ofb
        from oracle import tdnnf as otd
        r = ofb.fbank(wav, 80)
        r = otd.pad_input(r - r.mean(dim=1).unsqueeze(1), pad).permute(0, 2, 1)
        bounded("fbank_cmvn_pad", t["feats"], r, 3e-4)
    c.ref = ref
    return c


def _vq_row(entry, tiled, tie):
    shapes = [(1, 16, 1, 5), (3, 256, 63, 48), (1, 40, 64, 64), (3, 24, 65, 33), (3, 256, 165, 48)]
    if tiled:
        shapes += [(1, 64, 65, 65), (3, 32, 129, 256), (1, 16, 70, 1024)]

    @row(entry, "dist", shapes)
    def _(B, D, T, n_codes):
        c = Case()
        z, cb = rand(B, D, T, seed=T), rand(n_codes, D, seed=n_codes + 1)
        c.inp("z", z)
        c.inp("codebook", cb)
        c.out("q", (B, D, T))
        c.out("idx", (B, T), I32, index=True)
        c.out("dist", (B, T, n_codes))
        if tie:
            c.inp("pair_dist", torch.cdist(cb.double(), cb.double()).float())
            c.inout("tie_count", torch.tensor([[0] * B, [2 ** 31 - 1] * B, [-1] * B], dtype=I32))
        fn = getattr(_L(), entry)

        def call(t):
            if tie:
                _ok(fn(P(t["z"]), P(t["codebook"]), P(t["q"]), P(t["idx"]), P(t["dist"]), P(t["pair_dist"]), 1e-3, P(t["tie_count"]), B, D, T, n_codes,
                       _stream()), entry)
            else:
                _ok(fn(P(t["z"]), P(t["codebook"]), P(t["q"]), P(t["idx"]), P(t["dist"]), B, D, T, n_codes, _stream()), entry)
        c.call = call

        def ref(t):      # tests/test_hip_parity.py::test_vq_matches_oracle: expanded-form f32 distances to 1e-3 at |z|^2 ~ 256, the gather to 1e-6
            zt = z.double().permute(0, 2, 1)
            d = ((zt[:, :, None, :] - cb.double()[None, None]) ** 2).sum(-1)
            bounded(entry + " dist", t["dist"], d, 1e-3 * max(1.0, D / 256))
            idx = t["idx"].cpu().long()
            assert int(idx.min()) >= 0 and int(idx.max()) < n_codes
            got_d = d.gather(2, idx.unsqueeze(-1)).squeeze(-1)
            assert bool((got_d - d.min(-1).values <= 2e-3 * max(1.0, D / 256)).all())
            bounded(entry + " q", t["q"], cb[idx].double().permute(0, 2, 1), 1e-6)
        c.ref = ref
        return c


_vq_row("sat_vq_argmin_gather_f32", False, False)
_vq_row("sat_vq_argmin_gather_tie_f32", False, True)
_vq_row("sat_vq_argmin_gather_tiled_f32", True, False)
_vq_row("sat_vq_argmin_gather_tiled_tie_f32", True, True)


# ---- F0 and the generator's input (csrc/bottleneck.hip, yaapt.hip) ---------------------------------------------------------------
def _f0_track(n, seed):
    g = torch.Generator().manual_seed(seed)
    f0 = 80.0 + 220.0 * torch.rand(n, generator=g)
    f0 = torch.where(torch.rand(n, generator=g) < 0.6, f0, torch.zeros(n))
    f0[0] = 123.0
    return f0


@row("sat_f0_stats_f32", "all", [63, 1023, 1024, 1025, 8007])
def _(n):
    c = Case()
    f0 = _f0_track(n, n)
    c.inp("f0", f0)
    c.out("stats", (2,))
    c.call = lambda t: _ok(_L().sat_f0_stats_f32(P(t["f0"]), n, P(t["stats"]), _stream()), "sat_f0_stats_f32")

    def ref(t):          # the bounds of tests/test_hip_small_kernels.py::test_f0_stats_and_normalisation
        _, a = ref64.f0_normalise(f0)
        cnt = a["count"]
        k = math.ceil(n / 1024) + 6 + 16 + 2
        d = torch.where(f0 != 0, f0.double() - a["mean"], torch.zeros(n, dtype=torch.float64))
        dmean = k * U * a["S1"] / cnt
        dS = (k + 2) * U * a["S2"] + cnt * dmean ** 2 + 2 * dmean * U * d.abs().sum()
        v = a["var"] + ref64.f32(1e-6)
        dv = dS / (cnt - 1) + U * a["var"] + U * v
        bounded("f0_stats mean", t["stats"][0], torch.as_tensor(a["mean"]), dmean)
        bounded("f0_stats std", t["stats"][1], torch.as_tensor(a["std"]), dv / (2 * a["std"]) + U * a["std"])
    c.ref = ref
    return c


@row("sat_f0_apply_f32", "normalise", [(63, 0, 0), (1023, 0, 0), (1024, 16, 1), (1025, 64, 1), (8007, 0, 1)])
def _(n, bins, noisy):
    c = Case()
    f0 = _f0_track(n, n + 1)
    stats = torch.tensor([190.0, 61.5])
    noise = rand(n, seed=n + 2)
    c.inout("f0", f0)
    c.inp("stats", stats)
    if noisy:
        c.inp("noise", noise)
    c.call = lambda t: _ok(_L().sat_f0_apply_f32(P(t["f0"]), n, P(t["stats"]), bins, P(t.get("noise")), _stream()), "sat_f0_apply_f32")

    def ref(t):          # (v - mean) / std: one rounding each (test_f0_stats_and_normalisation's bound with exact statistics).  Quantisation and noise act
        # on the normalised float32 values and are exact functions of them (the same test): torch's on the kernel's own normalised track, bit for bit
        want = torch.where(f0 != 0, (f0.double() - 190.0) / 61.5, torch.zeros(n, dtype=torch.float64))
        norm = f0.to(DEV)
        _ok(_L().sat_f0_apply_f32(P(norm), n, P(stats.to(DEV)), 0, None, _stream()), "sat_f0_apply_f32")
        norm = norm.cpu()
        bounded("f0_apply", norm, want, 2 * U * want.abs())
        q = torch.where(norm != 0, torch.round(norm * bins) / bins, torch.zeros(n)) if bins else norm
        assert torch.equal(t["f0"].cpu(), torch.where(q != 0, q + noise, torch.zeros(n)) if noisy else q)
        assert not t["f0"].cpu()[f0 == 0].any()
    c.ref = ref
    return c


@row("sat_f0_mean_reversion_f32", "all", [(1, 1, 0.5), (31, 32, 0.5), (32, 33, 1.0), (33, 2, 0.5), (300, 32, 0.25)])
def _(T, n, alpha):
    c = Case()
    x = rand(1, 1, T, seed=T) * (torch.rand(1, 1, T, generator=torch.Generator().manual_seed(T)) > 0.3)
    c.inp("f0", x)
    c.out("out", (1, 1, T))
    c.call = lambda t: _ok(_L().sat_f0_mean_reversion_f32(P(t["f0"]), P(t["out"]), T, C.c_float(alpha), n, _stream()), "sat_f0_mean_reversion_f32")

    def ref(t):          # tests/test_hip_small_kernels.py::test_f0_mean_reversion
        want, a = ref64.mean_reversion(x, alpha, n)
        bound = a["alpha"] * (n + 1) * U * a["S"] + U * ((a["one_minus_alpha"] * x.double()).abs() + (a["alpha"] * a["avg"]).abs()) + U * want.abs()
        bounded("f0_mean_reversion", t["out"], want, bound)
    c.ref = ref
    return c


@row("sat_assemble_input_f32", "all", [(1, 1, 1, 9, 0), (3, 48, 255, 251, 247), (1, 3, 256, 256, 1), (3, 48, 257, 500, 3), (3, 2, 549, 3, 0)])
def _(B, c_bn, T, T_f0, n_spk):
    c = Case()
    bn, f0 = rand(B, c_bn, T, seed=T), rand(B, 1, T_f0, seed=T_f0)
    spk = rand(B, n_spk, seed=3) if n_spk else None
    c.inp("bn", bn)
    c.inp("f0", f0)
    if n_spk:
        c.inp("spk", spk)
    c.out("x", (B, c_bn + 1 + n_spk, T))
    c.call = lambda t: _ok(_L().sat_assemble_input_f32(P(t["bn"]), P(t["f0"]), P(t.get("spk")), P(t["x"]), B, c_bn, T, T_f0, n_spk, _stream()),
                           "sat_assemble_input_f32")
    c.ref = lambda t: bounded("assemble_input", t["x"], ref64.assemble_input(bn, f0, spk), 0)
    return c


YAAPT_OPTS = {"frame_length": 35.0, "frame_space": 20.0, "nccf_thresh1": 0.25, "tda_frame_length": 25.0}


def _yaapt_row_len(plan, v):
    """the largest length <= v that may be a row of a batch under the plan's options: the zero extension of its last spectral frame is
    not negative and its tda frames equal its analysis frames (any length under YAAPT_OPTS).  The others are refused by f0.yaapt_ragged
    and flagged by the kernels (status 3 / 4); tests/test_hip_yaapt_options.py runs such rows through the C entry point"""
    from satools_amd import f0 as f0_hip
    while True:
        _, L, nf, nt = f0_hip.length_dims(plan, v)
        if nt == nf and plan.nframe_size + (nf - 1) * plan.frame_jump >= L:
            return v
        v -= 1


def _yaapt_case(B, n, ragged, opts=YAAPT_OPTS, statuses=(0,)):
    from satools_amd import f0 as f0_hip
    from satools_amd import synthetic
    c = Case()
    plan = f0_hip.make_plan(n, dict(opts))
    wav = synthetic.harm_batch(list(range(B)), n)
    lens = [_yaapt_row_len(plan, n - 1237 * b) for b in range(B)]
    if ragged:
        for b in range(B):
            wav[b, lens[b]:] = 0.0
    nws = _L().sat_yaapt_workspace_bytes(C.byref(plan), B)
    hann = torch.hann_window(plan.frame_size + 2)[1:-1].contiguous()
    kaiser = torch.kaiser_window(plan.nframe_size, periodic=True, beta=0.5)
    k = np.arange(4096, dtype=np.float64)
    tw = torch.from_numpy(np.stack([np.cos(2 * np.pi * k / 8192.0), -np.sin(2 * np.pi * k / 8192.0)], 1).astype(np.float32))
    c.inp("wav", wav)
    c.inp("hann", hann)
    c.inp("kaiser", kaiser)
    c.inp("twiddle", tw)
    if ragged:
        c.inp("utt_dims", torch.tensor([f0_hip.length_dims(plan, v) for v in lens], dtype=I32), index=True)
    c.out("f0", (B, plan.nframes))
    c.out("status", (B,), I32)
    # the workspace: scratch, except its first B x 2 x Lz floats — the two filtered signals, whose zero extension past an utterance's padded
    # length the FFT frames read: an owned output (f0.workspace_views: "filt")
    filt = B * 2 * plan.Lz * 4
    assert filt <= nws
    c.out("ws", (nws,), U8, free=mask_of((nws,), slice(filt, None)))
    fn = _L().sat_yaapt_ragged_f32 if ragged else _L().sat_yaapt_f32

    def call(t):
        args = [C.byref(plan), P(t["wav"])] + ([P(t["utt_dims"])] if ragged else []) + [P(t["f0"]), P(t["status"]), P(t["hann"]), P(t["kaiser"]), P(t["twiddle"]),
                                                                                     P(t["ws"]), nws, B, _stream()]
        _ok(fn(*args), "sat_yaapt")
    c.call = call

    def ref(t):          # a whole pipeline: the plain call is its reference (property E); here only that it tracked something
        assert set(t["status"].cpu().tolist()) == set(statuses) and bool(torch.isfinite(t["f0"]).all())
    c.ref = ref
    return c


@row("sat_yaapt_f32", "harmonic", [(1, 8000), (3, 16123)])
def _(B, n):
    return _yaapt_case(B, n, False)


@row("sat_yaapt_ragged_f32", "harmonic", [(1, 8000), (3, 16123)])
def _(B, n):
    return _yaapt_case(B, n, True)


# the option sets of tests/yaapt_cases.py that move a buffer extent or a loop limit (the plan fields are asserted on the CPU by
# tests/test_yaapt_cases_host.py): nframe_size 1280 with an overlap of 128; tda_len 1024 (lengths with n mod 896 in 384..640: the
# reference's zero extension is not negative and the tda frames equal the analysis frames); an overlap of 1; short frames; 8 kHz; the
# largest harmonic count; and the set whose NCCF windows are empty (status 2: the kernel's guard, not its loops, must hold)
def _yaapt_option_rows(set_name, shapes, statuses=(0,)):
    def opts():
        import yaapt_cases
        return yaapt_cases.option_set(set_name).opts
    for entry, ragged in (("sat_yaapt_f32", False), ("sat_yaapt_ragged_f32", True)):
        row(entry, "harmonic/" + set_name, shapes)(lambda B, n, ragged=ragged: _yaapt_case(B, n, ragged, opts(), statuses))


_yaapt_option_rows("jump512_ov128", [(1, 8192), (3, 16901)])
_yaapt_option_rows("tda1024", [(1, 9 * 896 + 512), (3, 18 * 896 + 400)])
_yaapt_option_rows("ov1", [(1, 8000), (3, 16123)])
_yaapt_option_rows("short", [(1, 8000), (3, 16123)])
_yaapt_option_rows("sr8000", [(1, 8000), (3, 16123)])
_yaapt_option_rows("nharm6_f0max250", [(1, 8000), (3, 16123)])
_yaapt_option_rows("status2", [(1, 8000), (3, 16123)], statuses=(2,))      # the float32 oracle asserts on every row and length


# ---- wav2vec2 support (csrc/w2v2.hip) ----------------------------------------------------------------------------------------------
def _conv0_params(Cc=512, k=10):
    return rand(Cc, k, seed=2, scale=0.3), rand(Cc, seed=3, scale=0.1), 1 + rand(Cc, seed=4, scale=0.1), rand(Cc, seed=5, scale=0.1)


def _ln_ref(y, g, beta, gelu, split):
    r = F.layer_norm(y.double().transpose(1, 2), (y.shape[1],), g.double(), beta.double(), 1e-5).transpose(1, 2)
    if gelu:
        r = F.gelu(r)
    if split:
        ev, od = r[:, :, 0::2], r[:, :, 1::2]
        r = torch.cat([ev, F.pad(od, (0, ev.shape[2] - od.shape[2]))], 1)          # the odd-length zero slot is owned output
    return r


@row("sat_w2v2_conv0_f32", "k10s5", [(1, 10), (3, 10 + 5 * 254), (1, 10 + 5 * 255), (3, 10 + 5 * 256 + 3), (3, 4005)])       # 256 frames per block
def _(B, n):
    c = Case()
    x = rand(B, n, seed=n, scale=0.3)
    w, b, _, _ = _conv0_params()
    T = (n - 10) // 5 + 1
    c.inp("x", x)
    c.inp("w", w)
    c.inp("bias", b)
    c.out("y", (B, 512, T))
    c.call = lambda t: _ok(_L().sat_w2v2_conv0_f32(P(t["x"]), P(t["w"]), P(t["bias"]), P(t["y"]), B, n, 512, 10, 5, _stream()), "sat_w2v2_conv0_f32")
    # tests/test_hip_w2v2.py::test_conv0_and_layernorm_phase_split: 1e-5
    c.ref = lambda t: bounded("w2v2_conv0", t["y"], F.conv1d(x.double().unsqueeze(1), w.double().unsqueeze(1), b.double(), stride=5), 1e-5)
    return c


def _ln_case(B, Cc, T, gelu, split, planes, want_f32, pitch=3):
    c = Case()
    x = rand(B, Cc + 2, T + pitch, seed=T, scale=3.0) + 0.5       # the input: a channel slice with a row pitch of a wider tensor
    live = mask_of(x.shape, slice(None), slice(1, Cc + 1), slice(0, T))
    g, beta = rand(Cc, seed=4), rand(Cc, seed=5)
    Co, To = (2 * Cc, (T + 1) // 2) if split else (Cc, T)
    c.inp("x", x, dontcare=~live)
    c.inp("gamma", g)
    c.inp("beta", beta)
    if want_f32:
        c.out("y", (B, Co, To))
    else:
        c.untouched("y", (B, Co, To))
    if planes:
        c.out("y_split", (B, Co // 16, 2, 2, To, 8), F16)

    def call(t):
        xv = t["x"][:, 1:Cc + 1, :T]
        if planes:
            _ok(_L().sat_layernorm_channels_planes_f32(P(xv), P(t["gamma"]), P(t["beta"]), P(t["y"]) if want_f32 else None, P(t["y_split"]), B, Cc, T,
                                                     xv.stride(0), xv.stride(1), Co * To, To, int(gelu), int(split), _stream()), "sat_layernorm_channels_planes_f32")
        else:
            _ok(_L().sat_layernorm_channels_f32(P(xv), P(t["gamma"]), P(t["beta"]), P(t["y"]), B, Cc, T, xv.stride(0), xv.stride(1), Co * To, To,
                                              int(gelu), int(split), _stream()), "sat_layernorm_channels_f32")
    c.call = call

    def ref(t):          # tests/test_hip_w2v2.py::test_layernorm_planes_equal_split_of_f32_output: 2e-5, planes = the split of the f32 values
        _, ops, _ = _sat()
        want = _ln_ref(x[:, 1:Cc + 1, :T], g, beta, gelu, split)
        if want_f32:
            bounded("layernorm_channels", t["y"], want, 2e-5)
            if planes:
                assert torch.equal(t["y_split"], ops.act_split(t["y"].contiguous(), 1.0))
        else:
            bounded("layernorm_channels planes", ops.unsplit(t["y_split"]), want, 2e-5 + 2.0 ** -21 * want.abs())
    c.ref = ref
    return c


LN_T = [(1, 1), (3, 31), (1, 32), (3, 33), (3, 101)]       # LN_FR = 32 frames per block


@row("sat_layernorm_channels_f32", "plain", [(b, 512, t, 0, 0) for b, t in LN_T] + [(b, 504, t, 1, 1) for b, t in LN_T])
def _(B, Cc, T, gelu, split):
    return _ln_case(B, Cc, T, gelu, split, False, True)


@row("sat_layernorm_channels_planes_f32", "planes", [(b, 512, t, 1, 1, 1) for b, t in LN_T] + [(b, 1024, t, 0, 0, 0) for b, t in LN_T])
def _(B, Cc, T, gelu, split, want_f32):
    return _ln_case(B, Cc, T, gelu, split, True, want_f32)


@row("sat_w2v2_conv0_layernorm_f32", "gelu+phases", [(1, 10, 1), (3, 10 + 5 * 30, 0), (1, 10 + 5 * 31, 1), (3, 10 + 5 * 32 + 3, 0), (3, 4005, 1)])
def _(B, n, want_f32):
    c = Case()
    x = rand(B, n, seed=n, scale=0.3)
    w, b, g, beta = _conv0_params()
    T = (n - 10) // 5 + 1
    Co, To = 1024, (T + 1) // 2
    for name, v in (("x", x), ("w", w), ("bias", b), ("gamma", g), ("beta", beta)):
        c.inp(name, v)
    if want_f32:
        c.out("y", (B, Co, To))
    else:
        c.untouched("y", (B, Co, To))
    c.out("y_split", (B, Co // 16, 2, 2, To, 8), F16)
    c.call = lambda t: _ok(_L().sat_w2v2_conv0_layernorm_f32(P(t["x"]), P(t["w"]), P(t["bias"]), P(t["gamma"]), P(t["beta"]), P(t["y"]) if want_f32 else None,
                                                            P(t["y_split"]), B, n, 512, 10, 5, Co * To, To, 1, 1, _stream()), "sat_w2v2_conv0_layernorm_f32")

    def ref(t):          # the two kernels it fuses, at their bars (1e-5 through a LayerNorm of unit gain, 2e-5)
        _, ops, _ = _sat()
        want = _ln_ref(F.conv1d(x.double().unsqueeze(1), w.double().unsqueeze(1), b.double(), stride=5), g, beta, True, True)
        bounded("w2v2_conv0_layernorm", ops.unsplit(t["y_split"]), want, 2e-5 + 2.0 ** -21 * want.abs())
        if want_f32:
            bounded("w2v2_conv0_layernorm f32", t["y"], want, 2e-5)
    c.ref = ref
    return c


@row("sat_softmax_columns_f32", "pitched", [(1, 1, 64), (6, 63, 64), (2, 64, 64), (6, 65, 128), (3, 249, 256)])
def _(G, T, pitch):
    c = Case()
    st = rand(G * T, pitch, seed=T, scale=4.0)
    pad = mask_of(st.shape, slice(None), slice(T, None))
    c.inout("st", st, dontcare=pad, free=pad)          # the pad columns (queries >= T) are nobody's: not read into a result, not looked at
    c.call = lambda t: _ok(_L().sat_softmax_columns_f32(P(t["st"]), G, T, pitch, 0.125, _stream()), "sat_softmax_columns_f32")

    def ref(t):          # tests/test_hip_w2v2.py::test_attention_as_grouped_convs: 2e-5 on the attention output; a softmax weight is <= 1
        want = torch.softmax(st.double().view(G, T, pitch)[:, :, :T] * 0.125, dim=1)
        bounded("softmax_columns", t["st"].view(G, T, pitch)[:, :, :T], want, 2e-5)
    c.ref = ref
    return c


@row("sat_transpose_heads_f32", "pitched", [(1, 64, 1, 64), (6, 64, 15, 64), (2, 64, 16, 64), (6, 64, 17, 64), (3, 64, 249, 256)])
def _(G, D, T, pitch):
    c = Case()
    jpad = (T + 15) // 16 * 16
    v = rand(G, D, pitch, seed=T)
    c.inp("v", v, dontcare=mask_of(v.shape, slice(None), slice(None), slice(T, None)))
    c.out("vt", (G, jpad, D))                           # rows >= T are zero: owned output (the packed-weight layout a conv reads)
    c.call = lambda t: _ok(_L().sat_transpose_heads_f32(P(t["v"]), P(t["vt"]), G, D, T, pitch, jpad, _stream()), "sat_transpose_heads_f32")
    c.ref = lambda t: bounded("transpose_heads", t["vt"], F.pad(v[:, :, :T].transpose(1, 2), (0, 0, 0, jpad - T)), 0)
    return c


@row("sat_attention_f16x3", "f32+planes", [(1, 1, 1), (3, 31, 0), (1, 255, 1), (3, 256, 1), (1, 257, 0), (3, 549, 1)])
def _(B, T, want_f32):
    _, ops, _ = _sat()
    c = Case()
    heads, hd = 2, 64
    q, k, v = (rand(B, heads * hd, T, seed=T + i, scale=s) for i, s in enumerate((1.5, 1.5, 1.0)))
    pitch = (T + 63) // 64 * 64 if T > 256 else 256
    vp = F.pad(v, (0, pitch - T))
    c.inp("q_split", ops.act_split(q.to(DEV), 1.0))
    c.inp("k_split", ops.act_split(k.to(DEV), 1.0))
    c.inp("v", vp, dontcare=mask_of(vp.shape, slice(None), slice(None), slice(T, None)))      # v_pitch > T: uninitialised on the product path
    if want_f32:
        c.out("o", (B, heads * hd, T))
    else:
        c.untouched("o", (B, heads * hd, T))
    c.out("o_split", (B, heads * hd // 16, 2, 2, T, 8), F16)
    c.call = lambda t: _ok(_L().sat_attention_f16x3(P(t["q_split"]), P(t["k_split"]), P(t["v"]), P(t["o"]) if want_f32 else None, P(t["o_split"]), B, heads, hd, T,
                                                   pitch, hd ** -0.5, _stream()), "sat_attention_f16x3")

    def ref(t):          # tests/test_hip_w2v2.py::test_fused_attention_matches_float64: 1e-5 max, 1e-6 rms
        qd, kd, vd = (x.double().reshape(B, heads, hd, T) for x in (q, k, v))
        p = torch.softmax(torch.einsum("bhcq,bhcj->bhqj", qd, kd) * hd ** -0.5, dim=-1)
        want = torch.einsum("bhqj,bhdj->bhdq", p, vd).reshape(B, heads * hd, T)
        got = t["o"] if want_f32 else ops.unsplit(t["o_split"])
        bounded("attention_f16x3", got, want, 1e-5 + (0 if want_f32 else 2.0 ** -21 * want.abs()))
        assert float((got.cpu().double() - want).pow(2).mean().sqrt()) < 1e-6
        if want_f32:
            assert torch.equal(t["o_split"], ops.act_split(t["o"].contiguous(), 1.0))
    c.ref = ref
    return c


# ---- x-vector extractors and ASV scoring (csrc/xvector.hip, asv_score.hip, conv2d.hip) -----------------------------------------------
@row("sat_melspec_logmel_f32", "noise", [(1, 513), (3, 639), (1, 640), (3, 801), (3, 2011)])       # XV_FPB = 4 frames of 160 samples per block
def _(B, n):
    from satools_amd import xvector
    c = Case()
    wav = rand(B, n, seed=n, scale=0.3)
    window, fb = torch.hann_window(400, periodic=True), xvector.mel_filterbank().t().contiguous()
    nz = fb > 0
    lo = torch.where(nz.any(1), nz.float().argmax(1), torch.zeros(80, dtype=torch.long)).to(I32)
    hi = torch.where(nz.any(1), fb.shape[1] - torch.flip(nz, [1]).float().argmax(1), torch.zeros(80, dtype=torch.long)).to(I32)
    c.inp("wav", wav)
    c.inp("window", window)
    c.inp("fb", fb)
    c.inp("fb_lo", lo, index=True)
    c.inp("fb_hi", hi, index=True)
    c.out("out", (B, 80, 1 + n // 160))
    c.call = lambda t: _ok(_L().sat_melspec_logmel_f32(P(t["wav"]), P(t["out"]), P(t["window"]), P(t["fb"]), P(t["fb_lo"]), P(t["fb_hi"]), B, n, 80, 0.97, _stream()),
                           "sat_melspec_logmel_f32")

    def ref(t):          # the bound of tests/test_hip_small_kernels.py::test_melspec_logmel, in the power domain
        mel, aux = ref64.melspec(wav, window, fb, 0.97)
        dX = 84 * U * aux["A"].unsqueeze(2)
        dP = 2 * aux["amp"] * dX + dX * dX + 3 * U * aux["power"]
        taps = (fb > 0).sum(1).double().view(1, -1, 1)
        dM = torch.matmul(dP, fb.double().t()).transpose(1, 2) + (taps + 1) * U * mel
        cc = ref64.f32(1e-6)
        bounded("melspec_logmel", torch.exp(t["out"].cpu().double()), mel + cc, dM + (mel + cc) * (U + 2 * ULP * torch.log(mel + cc).abs()))
    c.ref = ref
    return c


RT = [(1, 1), (3, 63), (4, 64), (5, 65), (1027, 165)]       # one wave per row, four rows per block: lane tails and row tails


@row("sat_instnorm_rows_f32", "randn", RT)
def _(R, T):
    c = Case()
    x = rand(R, T, seed=T)
    c.inp("x", x)
    c.out("y", (R, T))
    c.call = lambda t: _ok(_L().sat_instnorm_rows_f32(P(t["x"]), P(t["y"]), R, T, 1e-5, _stream()), "sat_instnorm_rows_f32")

    def ref(t):          # the bound of tests/test_hip_small_kernels.py::test_instnorm_rows
        if T == 1:
            return bounded("instnorm_rows", t["y"], torch.zeros(R, 1), 0)
        k, eps = ref64.reduction_terms(T), 1e-5
        want, a = ref64.instance_norm(x, eps)
        d = x.double() - a["mean"]
        dmean = k * U * a["S1"] / T
        dd = dmean + U * d.abs()
        dq = (k + 2) * U * a["S2"] + T * dmean ** 2 + 2 * dmean * U * d.abs().sum(-1, keepdim=True)
        v = a["var"] + ref64.f32(eps)
        dv = dq / T + U * a["var"] + U * v
        rstd = 1.0 / torch.sqrt(v)
        drstd = torch.maximum(1.0 / torch.sqrt((v - dv).clamp(min=1e-300)) - rstd, rstd - 1.0 / torch.sqrt(v + dv)) + 2 * U * rstd
        bounded("instnorm_rows", t["y"], want, dd * (rstd + drstd) + d.abs() * drstd + U * want.abs())
    c.ref = ref
    return c


@row("sat_row_mean_f32", "randn", RT)
def _(R, T):
    c = Case()
    x = rand(R, T, seed=T + 1)
    c.inp("x", x)
    c.out("y", (R, 1))
    c.call = lambda t: _ok(_L().sat_row_mean_f32(P(t["x"]), P(t["y"]), R, T, _stream()), "sat_row_mean_f32")

    def ref(t):          # tests/test_hip_small_kernels.py::test_row_mean
        want, a = ref64.row_mean(x)
        bounded("row_mean", t["y"], want.reshape(R, 1), (ref64.reduction_terms(T) * U * a["S1"] / T).reshape(R, 1))
    c.ref = ref
    return c


@row("sat_l2norm_rows_f32", "randn", RT)
def _(R, D):
    c = Case()
    x = rand(R, D, seed=D + 2)
    x[::2] *= 0.0 if R > 4 else 1.0
    c.inp("x", x)
    c.out("y", (R, D))
    c.call = lambda t: _ok(_L().sat_l2norm_rows_f32(P(t["x"]), P(t["y"]), R, D, _stream()), "sat_l2norm_rows_f32")

    def ref(t):          # tests/test_hip_small_kernels.py::test_l2norm_rows
        want, a = ref64.l2norm(x)
        nrm = a["nrm"].clamp(min=1e-300)
        dn = ref64.reduction_terms(D) * U * a["S"] / (2 * nrm) + U * nrm
        bounded("l2norm_rows", t["y"], want, want.abs() * (dn / nrm + U))
    c.ref = ref
    return c


@row("sat_add3_f32", "channel slices", [(1, 1, 1, 0), (3, 3, 255, 1), (1, 5, 256, 0), (3, 4, 257, 1), (3, 3, 549, 1)])
def _(B, Cc, T, with_c):
    c = Case()
    pitch = T + 3

    def sl(ctot, c0, seed):
        buf = rand(B, ctot, pitch, seed=seed)
        return buf, (slice(None), slice(c0, c0 + Cc), slice(0, T))
    (a, asl), (b, bsl), (cc, csl) = sl(2 * Cc + 1, 1, 1), sl(Cc + 2, 2, 2), sl(3 * Cc, Cc, 3)
    ysl = (slice(None), slice(2 * Cc, 3 * Cc), slice(0, T))
    yshape = (B, 3 * Cc + 1, pitch)
    c.inp("a", a, dontcare=~mask_of(a.shape, *asl))
    c.inp("b", b, dontcare=~mask_of(b.shape, *bsl))
    if with_c:
        c.inp("c", cc, dontcare=~mask_of(cc.shape, *csl))
    c.out("y", yshape, untouched=~mask_of(yshape, *ysl))

    def call(t):
        av, bv, yv = t["a"][asl], t["b"][bsl], t["y"][ysl]
        cv = t["c"][csl] if with_c else None
        _ok(_L().sat_add3_f32(P(av), P(bv), P(cv), P(yv), B, Cc, T, av.stride(0), av.stride(1), bv.stride(0), bv.stride(1), cv.stride(0) if with_c else 0,
                              cv.stride(1) if with_c else 0, yv.stride(0), yv.stride(1), _stream()), "sat_add3_f32")
    c.call = call

    def ref(t):
        want = a[asl] + b[bsl]
        bounded("add3", t["y"][ysl], (want + cc[csl]) if with_c else want, 0)
    c.ref = ref
    return c


@row("sat_se_gate_add_f32", "sliced output", [(1, 1, 1, 0), (3, 5, 255, 1), (1, 7, 256, 2), (3, 5, 257, 3), (3, 5, 549, 3)])
def _(B, Cc, T, n_skips):
    c = Case()
    z, logits = rand(B, Cc, T, seed=T), rand(B, Cc, seed=T + 1, scale=3.0)
    skips = [rand(B, Cc, T, seed=T + 2 + i) for i in range(n_skips)]
    ysl = (slice(None), slice(Cc + 1, 2 * Cc + 1), slice(None))
    yshape = (B, 2 * Cc + 3, T)
    c.inp("z", z)
    c.inp("g", logits)
    for i, s in enumerate(skips):
        c.inp(f"s{i + 1}", s)
    c.out("y", yshape, untouched=~mask_of(yshape, *ysl))

    def call(t):
        yv = t["y"][ysl]
        _ok(_L().sat_se_gate_add_f32(P(t["z"]), P(t["g"]), P(t.get("s1")), P(t.get("s2")), P(t.get("s3")), P(yv), B, Cc, T, yv.stride(0), yv.stride(1), _stream()),
            "sat_se_gate_add_f32")
    c.call = call

    def ref(t):          # tests/test_hip_small_kernels.py::test_se_gate_add
        want, a = ref64.se_gate_add(z, logits, skips)
        bounded("se_gate_add", t["y"][ysl], want, a["prod"] * (1 * ULP + 2 * U + U) + U * a["partials"] + 2.0 ** -126 * z.double().abs())
    c.ref = ref
    return c


@row("sat_tanh_inplace_f32", "all", [1, 255, 256, 257, 4099])
def _(n):
    c = Case()
    x = rand(n, seed=n, scale=3.0)
    c.inout("x", x)
    c.call = lambda t: _ok(_L().sat_tanh_inplace_f32(P(t["x"]), n, _stream()), "sat_tanh_inplace_f32")

    def ref(t):          # tests/test_hip_small_kernels.py::test_tanh_inplace
        want = ref64.tanh(x)
        bounded("tanh_inplace", t["x"], want, 2 * ULP * want.abs() + 2.0 ** -149)
    c.ref = ref
    return c


@row("sat_attentive_stats_f32", "random", [(1, 1, 1), (3, 5, 63), (1, 4, 64), (3, 3, 65), (3, 5, 165)])
def _(B, Cc, T):
    import test_hip_small_kernels as sk
    c = Case()
    x, logits = rand(B, Cc, T, seed=T), rand(B, Cc, T, seed=T + 1, scale=2.0)
    c.inp("x", x)
    c.inp("logits", logits)
    c.out("out", (B, 2 * Cc, 1))
    c.call = lambda t: _ok(_L().sat_attentive_stats_f32(P(t["x"]), P(t["logits"]), P(t["out"]), B, Cc, T, _stream()), "sat_attentive_stats_f32")

    def ref(t):          # tests/test_hip_small_kernels.py::test_attentive_stats
        mean, std, a = ref64.attentive_stats(x, logits)
        dm1, dstd = sk._attentive_bounds(a, mean, std, T)
        bounded("attentive_stats mean", t["out"][:, :Cc, 0], mean, dm1)
        bounded("attentive_stats std", t["out"][:, Cc:, 0], std, dstd)
    c.ref = ref
    return c


@row("sat_res2_chain_f32", "dilated", [(1, 1, 1, 2), (3, 7, 127, 2), (1, 7, 128, 3), (3, 3, 129, 4), (3, 7, 293, 2)])
def _(B, nums, T, dil):
    c = Case()
    Cc = (nums + 1) * 64
    y = rand(B, Cc, T, seed=T)
    w = rand(nums, 3, 64, 64, seed=1, scale=(3 * 64) ** -0.5)
    scale, shift = 0.5 + torch.rand(nums, 64, generator=torch.Generator().manual_seed(2)), rand(nums, 64, seed=3, scale=0.1)
    c.inp("y", y)
    c.inp("w", w)
    c.inp("scale", scale)
    c.inp("shift", shift)
    c.out("z", (B, Cc, T))
    c.call = lambda t: _ok(_L().sat_res2_chain_f32(P(t["y"]), P(t["z"]), P(t["w"]), P(t["scale"]), P(t["shift"]), B, Cc, T, nums, dil, _stream()), "sat_res2_chain_f32")

    def ref(t):          # tests/test_hip_xvector.py::test_res2_chain_is_the_chain_of_convs: 5e-6 of the largest value, the last piece copied
        yd, prev, outs = y.double(), None, []
        for i in range(nums):
            xin = yd[:, 64 * i:64 * i + 64] + (prev if prev is not None else 0)
            prev = F.relu(F.conv1d(xin, w[i].double().permute(2, 1, 0), None, dilation=dil, padding=dil)) * scale[i].double()[None, :, None] + shift[i].double()[None, :, None]
            outs.append(prev)
        want = torch.cat(outs + [yd[:, 64 * nums:]], 1)
        bounded("res2_chain", t["z"], want, 5e-6 * max(1.0, float(want.abs().max())))
        assert torch.equal(t["z"][:, 64 * nums:].cpu(), y[:, 64 * nums:])
    c.ref = ref
    return c


@row("sat_linear_rows_f32", "epilogues", [(1, 1, 1, 0), (3, 63, 5, 1), (1, 64, 64, 0), (3, 65, 7, 1), (3, 2560, 129, 1)])
def _(B, cin, cout, full):
    c = Case()
    x, w = rand(B, cin, seed=cin), rand(cout, cin, seed=cout, scale=cin ** -0.5)
    b, sc, sh = rand(cout, seed=1), 0.5 + torch.rand(cout, generator=torch.Generator().manual_seed(2)), rand(cout, seed=3)
    c.inp("x", x)
    c.inp("w", w)
    if full:
        c.inp("bias", b)
        c.inp("ch_scale", sc)
        c.inp("ch_shift", sh)
    c.out("y", (B, cout))
    c.call = lambda t: _ok(_L().sat_linear_rows_f32(P(t["x"]), P(t["w"]), P(t.get("bias")), P(t.get("ch_scale")), P(t.get("ch_shift")), full, P(t["y"]), B, cin, cout,
                                                   _stream()), "sat_linear_rows_f32")

    def ref(t):          # tests/test_hip_xvector.py::test_linear_rows_is_the_linear_layer_on_pooled_vectors: 2e-6 of the largest value
        want = x.double() @ w.double().t()
        if full:
            want = F.relu(want + b.double()) * sc.double() + sh.double()
        bounded("linear_rows", t["y"], want, 2e-6 * max(1.0, float(want.abs().max())))
    c.ref = ref
    return c


@row("sat_cohort_topk_stats_f32", "rows", [(1, 1, 4, 1), (3, 200, 192, 200), (4, 257, 64, 30), (5, 1000, 256, 200), (7, 8192, 512, 200)])       # AS_ROWS = 4 rows per block
def _(N, Cn, D, k):
    c = Case()
    unit = lambda v: v / v.norm(dim=1, keepdim=True)
    x, coh = unit(rand(N, D, seed=N)), unit(rand(Cn, D, seed=Cn))
    c.inp("x", x)
    c.inp("cohort", coh)
    c.out("mean", (N,))
    c.out("std", (N,))
    c.call = lambda t: _ok(_L().sat_cohort_topk_stats_f32(P(t["x"]), P(t["cohort"]), N, Cn, D, k, P(t["mean"]), P(t["std"]), _stream()), "sat_cohort_topk_stats_f32")

    def ref(t):          # tests/test_hip_asv_score.py::test_cohort_topk_stats
        wm, ws, aux = ref64_asv.cohort_topk_stats(x, coh, k)
        bounded("cohort_topk_stats mean", t["mean"], wm, ref64_asv.topk_mean_bound(aux, Cn, D, k)[0])
        if k > 1:
            bounded("cohort_topk_stats std", t["std"], ws, ref64_asv.topk_std_bound(aux, ws, Cn, D, k))
    c.ref = ref
    return c


def _ip(t):
    return C.cast(t.data_ptr(), C.POINTER(C.c_int32))


@row("sat_trial_scores_f32", "cosine+asnorm", [(1, 1, 1, 4, 0), (3, 5, 255, 192, 1), (7, 2, 256, 64, 0), (5, 9, 257, 256, 1), (11, 13, 1029, 192, 1)])
def _(E, T, M, D, asnorm):
    c = Case()
    g = torch.Generator().manual_seed(M)
    enroll, test = rand(E, D, seed=E), rand(T, D, seed=T + 50)
    ie, it = torch.randint(0, E, (M,), generator=g).to(I32), torch.randint(0, T, (M,), generator=g).to(I32)
    stats = [rand(E, seed=1, scale=0.1), 0.5 + torch.rand(E, generator=g), rand(T, seed=2, scale=0.1), 0.5 + torch.rand(T, generator=g)]
    c.inp("enroll", enroll)
    c.inp("test", test)
    c.inp("idx_e", ie, index=True, host=True)           # HOST index lists: the entry checks them and copies them into idx_dev itself
    c.inp("idx_t", it, index=True, host=True)
    c.out("idx_dev", (2 * M,), I32, index=True)
    if asnorm:
        for n, s in zip(("mu_e", "sd_e", "mu_t", "sd_t"), stats):
            c.inp(n, s)
        c.out("score_asnorm", (M,))
    c.out("score", (M,))
    c.call = lambda t: _ok(_L().sat_trial_scores_f32(P(t["enroll"]), P(t["test"]), _ip(t["idx_e"]), _ip(t["idx_t"]), P(t["idx_dev"]), E, T, M, D, P(t.get("mu_e")),
                                                    P(t.get("sd_e")), P(t.get("mu_t")), P(t.get("sd_t")), P(t["score"]), P(t.get("score_asnorm")), _stream()),
                           "sat_trial_scores_f32")

    def ref(t):          # tests/test_hip_asv_score.py::test_trial_scores_cosine
        want, want_as, aux = ref64_asv.trial_scores(enroll, test, ie.tolist(), it.tolist(), stats if asnorm else None)
        ds = ref64_asv.score_bound(want, aux, D)
        bounded("trial_scores", t["score"], want, ds)
        if asnorm:          # tests/test_hip_asv_score.py::test_trial_scores_asnorm_from_device_statistics, the statistics given exactly here
            exact = [torch.zeros_like(v, dtype=torch.float64) for v in stats]
            bounded("trial_scores asnorm", t["score_asnorm"], want_as, ref64_asv.asnorm_bound(want, ds, stats, exact, ie.tolist(), it.tolist()))
        assert torch.equal(t["idx_dev"].cpu(), torch.cat([ie, it]))
    c.ref = ref
    return c


@row("sat_segment_mean_l2norm_f32", "segments", [(1, 1, 4), (7, 3, 192), (64, 9, 64), (65, 65, 256), (301, 17, 192)])
def _(Un, S, D):
    c = Case()
    g = torch.Generator().manual_seed(Un)
    x = rand(Un, D, seed=Un)
    order = torch.randperm(Un, generator=g).to(I32)
    cuts = sorted(torch.randperm(Un - 1, generator=g)[:S - 1].add(1).tolist()) if S > 1 else []
    offsets = torch.tensor([0] + cuts + [Un], dtype=I32)
    c.inp("x", x)
    c.inp("order", order, index=True, host=True)
    c.inp("offsets", offsets, index=True, host=True)
    c.out("seg_dev", (Un + S + 1,), I32, index=True)
    c.out("out", (S, D))
    c.call = lambda t: _ok(_L().sat_segment_mean_l2norm_f32(P(t["x"]), _ip(t["order"]), _ip(t["offsets"]), P(t["seg_dev"]), Un, S, D, P(t["out"]), _stream()),
                           "sat_segment_mean_l2norm_f32")

    def ref(t):          # tests/test_hip_asv_score.py::test_segment_mean_l2norm
        want, aux = ref64_asv.segment_mean_l2norm(x, order.numpy(), offsets.numpy())
        bounded("segment_mean_l2norm", t["out"], want, ref64_asv.segment_bound(want, aux, D))
    c.ref = ref
    return c


@row("sat_conv2d_f32", "mfma", [(1, 32, 32, 1, 1, 3, 1, "none"), (3, 64, 128, 3, 31, 3, 2, "affine_relu"), (1, 128, 128, 4, 32, 3, 1, "relu"), (3, 64, 128, 5, 33, 1, 2, "affine"),
                                (3, 32, 64, 9, 101, 3, 1, "affine_relu"), (1, 256, 256, 5, 33, 1, 1, "none"), (3, 1, 32, 5, 33, 3, 1, "affine_relu"), (1, 1, 32, 9, 101, 3, 1, "none")])
def _(B, cin, cout, H, W, ks, stride, epi):          # C2_TH = 4 output rows x C2_TW = 32 output columns per block
    _, ops, _ = _sat()
    c = Case()
    g = torch.Generator().manual_seed(H * W + cin)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * (cin * ks * ks) ** -0.5
    sc = (0.5 + torch.rand(cout, generator=g)) if "affine" in epi else None
    sh = torch.randn(cout, generator=g) if "affine" in epi else None
    relu = "relu" in epi
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    c.inp("x", x)
    c.inp("w", ops.pack_conv2d_weight(w))
    if sc is not None:
        c.inp("ch_scale", sc)
        c.inp("ch_shift", sh)
    c.out("y", (B, cout, Ho, Wo))
    c.family = "conv2d_stem_kernel" if cin == 1 else "conv2d_mfma_kernel"
    c.call = lambda t: _ok(_L().sat_conv2d_f32(P(t["x"]), P(t["w"]), P(t["y"]), P(t.get("ch_scale")), P(t.get("ch_shift")), int(relu), B, cin, cout, H, W, ks, stride,
                                              _stream()), "sat_conv2d_f32")

    def ref(t):          # tests/test_hip_xvector_resnet.py::_conv_case
        want, a = ref64_resnet.conv2d(x, w, stride, sc, sh, relu)
        kk = 9 * cin + 4
        if sc is None:
            bound = kk * U * a["S"]
        else:
            s64 = sc.double().view(1, -1, 1, 1)
            bound = kk * U * a["S"] * s64.abs() + U * (a["sum"] * s64).abs() + U * a["affine"].abs()
        bounded("conv2d", t["y"], want, bound)
    c.ref = ref
    return c


@row("sat_se_scale_add_relu_f32", "all", [(1, 1, 1), (3, 5, 255), (1, 7, 256), (3, 5, 257), (3, 32, 549)])
def _(B, Cc, N):
    c = Case()
    z, r, logits = rand(B, Cc, N, seed=N), rand(B, Cc, N, seed=N + 1), rand(B, Cc, seed=N + 2, scale=3.0)
    c.inp("z", z)
    c.inp("g", logits)
    c.inp("r", r)
    c.out("y", (B, Cc, N))
    c.call = lambda t: _ok(_L().sat_se_scale_add_relu_f32(P(t["z"]), P(t["g"]), P(t["r"]), P(t["y"]), B, Cc, N, _stream()), "sat_se_scale_add_relu_f32")

    def ref(t):          # tests/test_hip_xvector_resnet.py::test_se_scale_add_relu
        want, a = ref64_resnet.se_scale_add_relu(z, logits, r)
        bounded("se_scale_add_relu", t["y"], want, a["prod"] * (1 * ULP + 2 * U + U) + U * a["pre"].abs() + 2.0 ** -126 * z.double().abs())
    c.ref = ref
    return c


@row("sat_row_mean_std_f32", "randn", [(1, 1, 2), (3, 5, 63), (1, 4, 64), (3, 3, 65), (3, 2560, 19), (3, 3, 165)])
def _(B, Cc, T):
    import test_hip_xvector_resnet as xr
    c = Case()
    x = rand(B, Cc, T, seed=T)
    c.inp("x", x)
    c.out("out", (B, 2 * Cc))
    c.call = lambda t: _ok(_L().sat_row_mean_std_f32(P(t["x"]), P(t["out"]), B, Cc, T, _stream()), "sat_row_mean_std_f32")

    def ref(t):          # tests/test_hip_xvector_resnet.py::test_row_mean_std
        mean, std, a = ref64_resnet.mean_std(x)
        dm, ds = xr._mean_std_bounds(x, mean, std, a)
        bounded("row_mean_std mean", t["out"][:, :Cc], mean, dm)
        bounded("row_mean_std std", t["out"][:, Cc:], std, ds)
    c.ref = ref
    return c


# ---- the fused 1-D convolution in every arithmetic and layout it dispatches (csrc/conv1d_api.hip: conv1d_mfma.hip, conv_f16x3.hip, conv_lean.hip,
# conv_ring16.hip, gemm_ring.hip, gemm_walk16.hip) ------------------------------------------------------------------------------
def _pack(w, mode, **kw):
    """packed weights (on the device, as the product packs them) and the attributes that travel with the tensor"""
    _, _, packing = _sat()
    wd = w.to(DEV)
    pack = {0: packing.pack_conv_weight, 1: packing.pack_conv_weight_f16x3, 2: packing.pack_conv_weight_f16f8, 3: packing.pack_conv_weight_f16f8r}[mode]
    wp = pack(wd, **kw)
    return wp, {k: getattr(wp, k) for k in ("w_descale", "up_zero_taps") if hasattr(wp, k)}


def _attrs(t, attrs):
    for k, v in attrs.items():
        setattr(t, k, v)
    return t


def _lrelu(v, slope):
    return v if slope is None else F.leaky_relu(v, slope)


def conv_want(pre, w, b, r, sc, sh, acc0, T_q, *, cin, dil=1, stride=1, pads=(0, 0), groups=1, res_toff=0, res_tstride=1, res_scale=1.0, post_res=False, accum=False,
              accum_div=0.0, affine=False, relu=False, gelu=False, relu_first=False, wrap=0):
    """the float64 value conv_case holds a call to, in the order of sat_conv1d_desc's epilogue (include/satools_hip.h); pre = pre(x) in float64, r = the
    residual or None.  No GPU: tests/test_ref64_conv.py compares it with tests/ref64_conv.py on every row of CONV_ROWS"""
    if wrap:
        nxt = F.pad(pre[:, :cin - wrap, 1:], (0, 1))
        v = F.conv1d(pre, w[:, :wrap].double(), b.double()) + F.conv1d(nxt, w[:, wrap:].double())
    else:
        v = F.conv1d(F.pad(pre, pads), w.double(), b.double(), stride=stride, dilation=dil, groups=groups)[..., :T_q]
    rd = None if r is None else r.double()
    if rd is not None and not post_res:
        v = v + res_scale * rd[:, :, res_toff::res_tstride][..., :T_q]
    if relu and relu_first:
        v = F.relu(v)
    if affine:
        v = v * sc.double()[None, :, None] + sh.double()[None, :, None]
    if relu and not relu_first:
        v = F.relu(v)
    if gelu:
        v = F.gelu(v)
    if post_res:
        v = v + rd
    if accum:
        v = acc0.double()[..., :T_q] + v
        if accum_div:
            v = v / accum_div
    return v


def conv_case(B, T, cin, cout, k, *, mode=0, dil=1, stride=1, pads=None, groups=1, x_planes=False, slope=None, y_planes=False, no_y=False, sidecar=False,
              hi_only=False, res=None, res_toff=0, res_tstride=1, res_scale=1.0, post_res=False, accum=False, accum_div=0.0, affine=False, relu=False,
              gelu=False, relu_first=False, ypitch=0, wrap=0, family=None, options=(), bound=3e-5, x=None):
    """one sat_conv1d_f32 call.  `bound`: 3e-5 absolute on these O(1) outputs, the bar of tests/test_hip_parity.py::test_conv1d_matches_torch and
    ::test_conv1d_split_f16_matches_torch (exact f32 and split-f16 alike); SAT_CONV_F16F8R: 1e-4 of the scale, tests/test_hip_f8r.py"""
    _, ops, _ = _sat()
    c = Case(family=family, options=tuple(options))
    halo = dil * (k - 1)
    pl, pr = pads if pads is not None else (halo // 2, halo - halo // 2)
    cx = wrap or cin
    T_q = T if wrap else (T + pl + pr - halo - 1) // stride + 1
    x = rand(B, cx, T, seed=T + cin) if x is None else x          # (`x`: a given input, a sub-batch of another case's)
    c.data["x"] = x
    w = rand(cout, cin // groups, k, seed=2, scale=(cin // groups * k) ** -0.5)
    b = rand(cout, seed=3)
    wp, attrs = _pack(w, mode, **({"groups": groups} if mode != 3 else {}))
    xs = None
    if x_planes:
        xs = ops.act_split(x.to(DEV), 1.0 if slope is None else slope, fmt=1 if mode == 2 else 0)
        c.inp("x_split", xs)
        c.untouched("x", (B, cx, T))                    # with x_split, x only gives the shape: never read
        if mode == 3:
            c.inp("x_split8", ops.planes_f8_sidecar(xs))
    else:
        c.inp("x", x)
    c.inp("w", wp)
    c.inp("bias", b)
    yshape = (B, cout, T_q + ypitch)
    ypad = mask_of(yshape, slice(None), slice(None), slice(T_q, None)) if ypitch else None
    acc0 = rand(*yshape, seed=5)
    if no_y:
        c.untouched("y", yshape)
    elif accum:
        c.inout("y", acc0, untouched=ypad)
    else:
        c.out("y", yshape, untouched=ypad)
    r = None
    if res == "f32":
        r = rand(B, cout, (T_q - 1) * res_tstride + res_toff + 1, seed=4)
        c.inp("res", r)
    elif res == "planes":
        r = rand(B, cout, T_q, seed=4)
        c.inp("res_split", ops.act_split(r.to(DEV), 0.1))
    sc, sh = rand(cout, seed=9).abs() + 0.5, rand(cout, seed=10)
    if affine:
        c.inp("ch_scale", sc)
        c.inp("ch_shift", sh)
    if y_planes:
        pshape = (B, cout // 16, 2, 2, T_q, 8)
        c.out("y_split", pshape, F16, untouched=mask_of(pshape, slice(None), slice(None), 1) if hi_only else None)
    if sidecar:
        c.out("y_split8", (B, cout // 16, 2, T_q, 16), U8)

    def call(t, hi_only=hi_only):
        kw = dict(bias=t["bias"], dilation=dil, stride=stride, pad_left=pl, pad_right=pr, groups=groups, mode=mode, out=t["y"][:, :, :T_q], accum=accum,
                  accum_div=accum_div, relu=relu, gelu=gelu, x_split=t.get("x_split"), x_split8=t.get("x_split8"), y_split=t.get("y_split"),
                  y_split8=t.get("y_split8"), y_split_hi_only=hi_only, y_split_slope=0.1, no_y=no_y, res_split=t.get("res_split"), res_split_slope=0.1,
                  ch_scale=t.get("ch_scale"), ch_shift=t.get("ch_shift"), relu_first=relu_first)
        if res == "f32":
            kw.update(post_res=t["res"]) if post_res else kw.update(res=t["res"], res_scale=res_scale, res_toff=res_toff, res_tstride=res_tstride)
        if slope is not None and not x_planes:
            kw["in_lrelu"] = slope
        if wrap:
            kw.update(x_wrap_channels=wrap, c_in=cin, t_out=T)
        ops.conv1d(t["x"], _attrs(t["w"], attrs), cout, k, **kw)
    c.call = call

    def ref(t):
        # (SAT_SPLIT_F16 planes: the 22 bits of pre(x) the kernel is given)
        pre = ops.unsplit(xs).double().cpu() if x_planes and mode != 2 else _lrelu(x.double(), slope)
        v = conv_want(pre, w, b, r, sc, sh, acc0, T_q, cin=cin, dil=dil, stride=stride, pads=(pl, pr), groups=groups, res_toff=res_toff, res_tstride=res_tstride,
                      res_scale=res_scale, post_res=post_res, accum=accum, accum_div=accum_div, affine=affine, relu=relu, gelu=gelu, relu_first=relu_first, wrap=wrap)
        bd = bound * max(1.0, float(v.abs().max())) if mode == 3 else bound
        if not no_y:
            bounded("conv1d y", t["y"][:, :, :T_q], v, bd)
        if y_planes and mode == 2:          # SAT_SPLIT_F8 planes out (tests/test_hip_parity.py: the format this mode reads)
            assert torch.equal(t["y_split"], ops.act_split(t["y"][:, :, :T_q].contiguous(), 0.1, fmt=1))
        elif y_planes and not hi_only:
            want = F.leaky_relu(v, 0.1)
            bounded("conv1d y_split", ops.unsplit(t["y_split"]), want, bd + 2.0 ** -21 * want.abs())
            if not no_y:
                assert torch.equal(t["y_split"], ops.act_split(t["y"][:, :, :T_q].contiguous(), 0.1))
            if sidecar:
                assert torch.equal(t["y_split8"], ops.planes_f8_sidecar(t["y_split"]))
        elif y_planes:          # hi-only planes: hi = f16(lrelu(v)) toward zero, 2^-10 of it short at the most; the sidecar is that of the FULL planes
            want = F.leaky_relu(v, 0.1)          # (tests/test_hip_f8r.py::test_f16f8r_matches_its_decomposition, its case 4): the same call with both units gives them
            s = t["y_split"]
            bounded("conv1d y_split hi", ops.unsplit(torch.stack([s[:, :, 0], torch.zeros_like(s[:, :, 0])], 2)), want, bd + 2.0 ** -10 * want.abs())
            full = dict(t, y_split=torch.zeros_like(s), y_split8=torch.zeros_like(t["y_split8"]) if sidecar else None)
            with _options(c.options):
                call(full, False)
            bounded("conv1d y_split", ops.unsplit(full["y_split"]), want, bd + 2.0 ** -21 * want.abs())
            assert torch.equal(s[:, :, 0], full["y_split"][:, :, 0])
            if sidecar:
                assert torch.equal(full["y_split8"], ops.planes_f8_sidecar(full["y_split"])) and torch.equal(t["y_split8"], full["y_split8"])
    c.ref = ref
    return c


CONV_ROWS = []          # (name, shapes, keyword arguments of conv_case) of every row conv_rows adds


def conv_rows(name, tile, family, shapes=None, **kw):
    CONV_ROWS.append((name, shapes or times(tile), dict(kw)))
    cin, cout, k = kw.pop("cin"), kw.pop("cout"), kw.pop("k")

    @row("sat_conv1d_f32", name, shapes or times(tile))
    def _(B, T):
        return conv_case(B, T, cin, cout, k, family=family, **kw)


RING = (("convring", 33, 1),)          # the LDS-DMA ring whatever the number of tiles (by default it wants three quarters of the CUs filled)
# exact f32 (conv1d_mfma_kernel): 64 x 256, 128 x 32 and 32 x 512 tiles
conv_rows("f32 k5 dilated 64x256", 256, "conv1d_mfma_kernel", cin=48, cout=40, k=5, dil=2)
conv_rows("f32 504->512 k7 128x32", 32, "conv1d_mfma_kernel", cin=504, cout=512, k=7)
conv_rows("f32 tdnnf epilogue res_toff res_tstride affine relu", 32, "conv1d_mfma_kernel", cin=32, cout=128, k=1, res="f32", res_toff=1, res_tstride=2, res_scale=0.66,
          affine=True, relu=True)
conv_rows("f32 groups 4 k16 32x512", 512, "conv1d_mfma_kernel", cin=128, cout=128, k=16, groups=4, pads=(8, 8))
conv_rows("f32 runtime taps k10 stride 5", 32, "conv1d_mfma_kernel", cin=64, cout=96, k=10, stride=5, pads=(0, 0),
          shapes=[(1, 10), (3, 10 + 5 * 30), (1, 10 + 5 * 31 + 2), (3, 10 + 5 * 32 + 4), (3, 10 + 5 * 100)])
conv_rows("f32 stride 2 k2", 32, "conv1d_mfma_kernel", cin=512, cout=512, k=2, stride=2, pads=(0, 0), shapes=[(1, 2), (3, 63), (1, 64), (3, 67), (3, 203)])
conv_rows("f32 groups 16 k128 gelu post_res", 512, "conv1d_mfma_kernel", cin=64, cout=64, k=128, groups=16, pads=(64, 63), gelu=True, res="f32", post_res=True)
conv_rows("f32 accum /3 res pitched y", 256, "conv1d_mfma_kernel", cin=64, cout=64, k=7, dil=3, slope=0.1, res="f32", accum=True, accum_div=3.0, ypitch=5)
# split-f16 from f32 input (conv1d_f16x3_kernel): 32 x 512 tiles, the generator's conv_pre on both widths of its tile
conv_rows("f16x3 f32-in k3 32x512", 512, "conv1d_f16x3_kernel", cin=16, cout=16, k=3, mode=1, slope=0.1, res="f32")
conv_rows("f16x3 conv_pre 80->512 k7 half-width tile", 128, "conv1d_f16x3_kernel", cin=80, cout=512, k=7, mode=1)
conv_rows("f16x3 conv_pre 80->512 k7 full tile", 256, "conv1d_f16x3_kernel", cin=80, cout=512, k=7, mode=1, options=(("half_tile7", 0, 1),))
conv_rows("f16x3 504->512 k7 f32-in", 256, "conv1d_f16x3_kernel", cin=504, cout=512, k=7, mode=1, slope=0.1, res="f32", options=(("half_tile7", 0, 1),))
conv_rows("f16x3 k2 f32-in", 256, "conv1d_f16x3_kernel", cin=48, cout=40, k=2, mode=1)
# planes in, planes out
# (the half-width tile is chosen at T > 128 only: the tile edges are 129, 255, 256, 257)
conv_rows("planes k3 half-width tile", 128, "conv1d_f16x3_kernel", cin=64, cout=64, k=3, mode=1, x_planes=True, slope=0.1, y_planes=True, no_y=True,
          shapes=[(1, 129), (3, 255), (1, 256), (3, 257), (3, 421)])
for _bal in (0, 1, 2):
    conv_rows(f"planes lean k7 lean_balance {_bal}", 256, "conv1d_f16x3_planes_lean_kernel", cin=64, cout=64, k=7, dil=3, mode=1, x_planes=True, slope=0.1, y_planes=True,
              res="planes", options=(("lean_balance", _bal, 1),), shapes=times(256) + [(3, 256 + 128), (3, 256 + 129)])
conv_rows("planes lean k11 accum /3", 256, "conv1d_f16x3_planes_lean_kernel", cin=64, cout=64, k=11, dil=5, mode=1, x_planes=True, slope=0.1, res="planes", accum=True,
          accum_div=3.0)
# (3 taps on planes at T > 128 with few blocks go to the half-width tile, the row "planes k3 half-width tile" above: the lean kernel sees T <= 128 only)
conv_rows("planes lean k3 no_y", 256, "conv1d_f16x3_planes_lean_kernel", cin=64, cout=64, k=3, dil=5, mode=1, x_planes=True, slope=0.1, y_planes=True, no_y=True,
          shapes=[(1, 1), (3, 127), (3, 128)])
conv_rows("planes lean off: 64x256 tile", 256, "conv1d_f16x3_kernel", cin=64, cout=64, k=7, mode=1, x_planes=True, slope=0.1, y_planes=True, res="planes",
          options=(("lean7", 0, 1),))
conv_rows("planes 32 rows k11", 512, "conv1d_f16x3_kernel", cin=32, cout=32, k=11, mode=1, x_planes=True, slope=0.1, y_planes=True, no_y=True)
# (SAT_CONV_F16F8: the lean kernel and the ring do not take the 8-bit planes, so the 64 x 256 tile)
conv_rows("f16f8 SPLIT_F8 planes k7 res", 256, "conv1d_f16x3_kernel", cin=64, cout=64, k=7, dil=3, mode=2, x_planes=True, slope=0.1, y_planes=True, res="f32", bound=1e-4)
# the LDS-DMA ring: 128 x 320 and 256 x 160 tiles, the 8-bit sidecar, hi-only planes, SAT_CONV_F16F8R with equal and unequal channel counts
conv_rows("ring 128 rows k3 sidecar", 320, "conv1d_f16x3_ring16_kernel", cin=128, cout=128, k=3, dil=5, mode=1, x_planes=True, slope=0.1, y_planes=True, no_y=True,
          sidecar=True, options=RING)
conv_rows("ring 256 rows k7 res accum", 160, "conv1d_f16x3_ring16_kernel", cin=256, cout=256, k=7, dil=3, mode=1, x_planes=True, slope=0.1, y_planes=True, res="planes",
          accum=True, accum_div=3.0, options=RING)
conv_rows("ring 128 rows k11 hi-only planes", 320, "conv1d_f16x3_ring16_kernel", cin=128, cout=128, k=11, mode=1, x_planes=True, slope=0.1, y_planes=True, no_y=True,
          sidecar=True, hi_only=True, options=RING)
F8FAM = "conv1d_f16x3_ring16_kernel (F8: 8-bit cross terms)"
conv_rows("f16f8r 128 k3 planes+sidecar", 320, F8FAM, cin=128, cout=128, k=3, mode=3, x_planes=True, slope=0.1, y_planes=True, no_y=True, sidecar=True, bound=1e-4)
conv_rows("f16f8r 256 k11 res f32+planes", 160, F8FAM, cin=256, cout=256, k=11, dil=5, mode=3, x_planes=True, slope=0.1, y_planes=True, res="planes", sidecar=True,
          bound=1e-4)
conv_rows("f16f8r 96->160 k7 accum", 160, F8FAM, cin=96, cout=160, k=7, dil=3, mode=3, x_planes=True, slope=0.1, res="planes", accum=True, accum_div=3.0, bound=1e-4)
conv_rows("f16f8r 160->96 k3", 320, F8FAM, cin=160, cout=96, k=3, mode=3, x_planes=True, slope=0.1, y_planes=True, bound=1e-4)
# 1x1 convs on split planes: the four GEMM kernels (128 x 256 tiles; 128 x 128 for the plain one).  The three 128 x 256 rows have no T = 1 and no T = 257:
# the dispatch gives those lengths to the 128 x 128 kernel (256-column tiles would pad them by more than an eighth), whose own row below has them
conv_rows("k1 ring16 gemm", 256, "gemm_f16x3_ring16_kernel", cin=128, cout=256, k=1, mode=1, x_planes=True, y_planes=True, res="f32", shapes=[(1, 255), (3, 256), (3, 677)])
conv_rows("k1 walk gemm gelu", 256, "gemm_f16x3_walk16_kernel", cin=128, cout=256, k=1, mode=1, x_planes=True, y_planes=True, gelu=True, options=(("gemm_walk", 3, 1),),
          shapes=[(1, 255), (3, 256), (3, 677)])
conv_rows("k1 ring gemm 32x32x16", 256, "gemm_f16x3_ring_kernel", cin=128, cout=256, k=1, mode=1, x_planes=True, y_planes=True, affine=True, relu=True,
          options=(("k1_gemm", 2, 3),), shapes=[(1, 255), (3, 256), (3, 677)])
conv_rows("k1 128x128 gemm", 128, "conv1d_f16x3_k1_kernel", cin=64, cout=504, k=1, mode=1, x_planes=True, res="f32", res_toff=1, res_scale=0.66, affine=True, relu=True,
          shapes=[(1, 1), (3, 127), (1, 128), (3, 129), (3, 293 + 128)], options=(("k1_gemm", 1, 3),))
conv_rows("k1 conv tile (k1_gemm 0)", 256, "conv1d_f16x3_kernel", cin=64, cout=128, k=1, mode=1, x_planes=True, y_planes=True, options=(("k1_gemm", 0, 3),))
conv_rows("k1 stride 2 wrapped", 256, "gemm_f16x3_ring16_kernel", cin=192, cout=128, k=1, mode=1, x_planes=True, wrap=128, y_planes=True,
          shapes=[(1, 1), (3, 255), (1, 256), (3, 257), (3, 677)])


def pos_piece_case(B, T, pad_left, Cc=1024, groups=16, k=11, bound=3e-5):
    """one of the twelve shifted 11-tap pieces the split-f16 path makes of the wav2vec2 positional conv (wav2vec2.py: grouped, 16 groups, f32 input,
    pad_left = 64 - 11 s, pad_right = 10 - pad_left, `res` and `out` the SAME tensor from the second piece on): piece 0 (pad_left 64) has the bias and
    writes a fresh tensor, the last (pad_left -57) the GELU.  A negative pad_left starts the window right of the output frame; at these T the window
    lies wholly left of the sequence (64 at T <= 54), wholly right of it (-57 at T <= 57) or straddles an end (9, -2).  `bound`: conv_case's"""
    _, ops, _ = _sat()
    c = Case()
    first, last = pad_left == 64, pad_left == -57
    x = rand(B, Cc, T, seed=T + Cc)
    w = rand(Cc, Cc // groups, k, seed=2, scale=(Cc // groups * k) ** -0.5)
    b = rand(Cc, seed=3)
    y0 = rand(B, Cc, T, seed=5)
    wp, attrs = _pack(w, 1, groups=groups)
    c.inp("x", x)
    c.inp("w", wp)
    c.inp("bias", b)
    if first:
        c.out("y", (B, Cc, T))
    else:
        c.inout("y", y0)

    def call(t):
        ops.conv1d(t["x"], _attrs(t["w"], attrs), Cc, k, bias=t["bias"] if first else None, pad_left=pad_left, pad_right=k - 1 - pad_left, groups=groups, mode=1,
                   res=None if first else t["y"], gelu=last, out=t["y"])
    c.call = call

    def ref(t):
        xp = torch.zeros(B, Cc, T + k - 1, dtype=torch.float64)          # xp[i] = x[i - pad_left] where that is a frame: F.pad cannot crop more than there is
        for i in range(T + k - 1):
            if 0 <= i - pad_left < T:
                xp[:, :, i] = x[:, :, i - pad_left].double()
        v = F.conv1d(xp, w.double(), b.double() if first else None, groups=groups)
        if not first:
            v = v + y0.double()
        bounded(f"conv1d positional piece pad_left {pad_left}", t["y"], F.gelu(v) if last else v, bound)
    c.ref = ref
    return c


@row("sat_conv1d_f32", "f16x3 positional-conv piece groups 16 k11 res=out", [(2, T, pl) for T in (1, 10, 53, 64) for pl in (64, 9, -2, -57)])
def _(B, T, pad_left):
    return pos_piece_case(B, T, pad_left)


def ups_case(B, T, cin, cout, k, u, *, mode=0, planes=False, grouped=False, mask=0, sidecar=False, family=None, options=(), bound=3e-5):
    """ConvTranspose1d(k, stride u, padding (k - u) / 2) as the polyphase conv of sat_conv1d_f32 (up = u): f32 in and out, planes to planes through the
    LDS-transposed epilogue, or the phase-grouped rows of the ring (up_grouped, with and without the zero-tap mask)"""
    _, ops, packing = _sat()
    c = Case(family=family, options=tuple(options))
    x = rand(B, cin, T, seed=T + cin)
    w, b = rand(cin, cout, k, seed=2, scale=(cin * k / u) ** -0.5), rand(cout, seed=3)
    wc, kp, pl = packing.convtranspose_as_phase_conv(w.to(DEV), u, (k - u) // 2, grouped=grouped)
    wp = packing.pack_conv_weight(wc, up=u) if mode == 0 else packing.pack_conv_weight_f16x3(wc, up=u)
    attrs = {a: getattr(wp, a) for a in ("w_descale", "up_zero_taps") if hasattr(wp, a)}
    c.inp("w", wp)
    c.inp("bias", b)
    if planes:
        c.inp("x_split", ops.act_split(x.to(DEV), 0.1))
        c.untouched("x", (B, cin, T))
        c.untouched("y", (B, cout, T * u))
        c.out("y_split", (B, cout // 16, 2, 2, T * u, 8), F16)
        if sidecar:
            c.out("y_split8", (B, cout // 16, 2, T * u, 16), U8)
    else:
        c.inp("x", x)
        c.out("y", (B, cout, T * u))

    def call(t):
        kw = dict(bias=t["bias"], pad_left=pl, up=u, mode=mode, out=t["y"])
        if planes:
            kw.update(x_split=t["x_split"], y_split=t["y_split"], y_split8=t.get("y_split8"), y_split_slope=0.1, no_y=True, up_grouped=grouped, up_zero_taps=mask)
        else:
            kw.update(in_lrelu=0.1)
        ops.conv1d(t["x"], _attrs(t["w"], attrs), cout, kp, **kw)
    c.call = call

    def ref(t):          # tests/test_hip_parity.py::test_convtranspose_as_polyphase_conv (3e-5), ::test_stride4_upsampler_on_the_ring_with_rows_grouped_by_phase (4e-6)
        want = F.conv_transpose1d(F.leaky_relu(x.double(), 0.1), w.double(), b.double(), stride=u, padding=(k - u) // 2)
        if planes:
            bounded("upsampler planes", ops.unsplit(t["y_split"]), F.leaky_relu(want, 0.1), bound)
            if sidecar:
                assert torch.equal(t["y_split8"], ops.planes_f8_sidecar(t["y_split"]))
        else:
            bounded("upsampler f32", t["y"], want, bound)
    c.ref = ref
    return c


def ups_rows(name, tile, family, cin, cout, k, u, **kw):
    @row("sat_conv1d_f32", name, times(tile))
    def _(B, T):
        return ups_case(B, T, cin, cout, k, u, family=family, **kw)


ups_rows("f32 up 2", 256, "conv1d_mfma_kernel", 64, 32, 4, 2)
ups_rows("f32 up 4 k8", 32, "conv1d_mfma_kernel", 128, 64, 8, 4)
ups_rows("f32 up 5 k11", 32, "conv1d_mfma_kernel", 64, 32, 11, 5)
ups_rows("planes up 2", 256, "conv1d_f16x3_kernel", 64, 32, 4, 2, mode=1, planes=True)
ups_rows("planes up 4", 256, "conv1d_f16x3_kernel", 128, 64, 8, 4, mode=1, planes=True)
ups_rows("planes up_grouped zero-tap mask", 160, "conv1d_f16x3_ring16_kernel", 256, 128, 8, 4, mode=1, planes=True, grouped=True, mask=0x30c, bound=4e-6)
ups_rows("planes up_grouped all taps sidecar", 160, "conv1d_f16x3_ring16_kernel", 128, 64, 8, 4, mode=1, planes=True, grouped=True, mask=0, sidecar=True, bound=4e-6)


# ---- several convs in one call ---------------------------------------------------------------------------------------------------
def multi_ring_case(B, T):
    """three ring jobs of one launch chained through the MRF sum (index order inside a block: no rotation)"""
    _, ops, _ = _sat()
    Cc, ks, dils = 128, (3, 7, 11), (1, 3, 5)
    c = Case(family="conv1d_f16x3_ring16_kernel", options=RING)
    x = rand(B, Cc, T, seed=T)
    xs = ops.act_split(x.to(DEV), 0.1)
    ws = [rand(Cc, Cc, k, seed=10 + k, scale=(k * Cc) ** -0.5) for k in ks]
    bs = [rand(Cc, seed=20 + k) for k in ks]
    attrs = []
    c.inp("x_split", xs)
    c.untouched("x", (B, Cc, T))
    for j, k in enumerate(ks):
        wp, a = _pack(ws[j], 1)
        attrs.append(a)
        c.inp(f"w{j}", wp)
        c.inp(f"b{j}", bs[j])
    c.out("acc", (B, Cc, T))
    c.out("y_split", (B, Cc // 16, 2, 2, T, 8), F16)

    def call(t):
        jobs = []
        for j, k in enumerate(ks):
            kw = dict(bias=t[f"b{j}"], dilation=dils[j], pad_left=dils[j] * (k - 1) // 2, mode=1, x_split=t["x_split"], y_split_slope=0.1, res_split=t["x_split"],
                      res_split_slope=0.1, out=t["acc"], accum=j > 0, accum_div=3.0 if j == 2 else 0.0, y_split=t["y_split"] if j == 2 else None)
            jobs.append((t["x"], _attrs(t[f"w{j}"], attrs[j]), Cc, k, kw))
        ops.conv1d_multi(jobs)
    c.call = call

    def ref(t):          # the single convs' bar (3e-5), three of them summed and divided by 3
        pre = ops.unsplit(xs).double().cpu()
        xr = torch.where(pre > 0, pre, pre * 10.0)
        v = sum(F.conv1d(pre, ws[j].double(), bs[j].double(), dilation=dils[j], padding=dils[j] * (k - 1) // 2) + xr for j, k in enumerate(ks)) / 3
        bounded("conv1d_multi ring", t["acc"], v, 3e-5)
        assert torch.equal(t["y_split"], ops.act_split(t["acc"].contiguous(), 0.1))
    c.ref = ref
    return c


row("sat_conv1d_multi_f32", "three ring jobs chained through the MRF sum", [(1, 1), (3, 319), (1, 320), (3, 321), (3, 677)])(multi_ring_case)


@row("sat_conv1d_multi_f32", "q | k | v on the persistent GEMM", [(1, 255), (3, 256), (3, 677)])
def _(B, T):
    _, ops, _ = _sat()
    cin, cout = 128, 256
    c = Case(family="gemm_f16x3_walk16_kernel")
    x = rand(B, cin, T, seed=T)
    xs = ops.act_split(x.to(DEV), 1.0)
    ws = [rand(cout, cin, 1, seed=30 + j, scale=cin ** -0.5) for j in range(3)]
    bs = [rand(cout, seed=40 + j) for j in range(3)]
    attrs = []
    c.inp("x_split", xs)
    c.untouched("x", (B, cin, T))
    for j in range(3):
        wp, a = _pack(ws[j], 1)
        attrs.append(a)
        c.inp(f"w{j}", wp)
        c.inp(f"b{j}", bs[j])
        c.out(f"y{j}", (B, cout, T)) if j == 2 else c.untouched(f"y{j}", (B, cout, T))
        c.out(f"ys{j}", (B, cout // 16, 2, 2, T, 8), F16)

    def call(t):
        ops.conv1d_multi([(t["x"], _attrs(t[f"w{j}"], attrs[j]), cout, 1, dict(bias=t[f"b{j}"], mode=1, x_split=t["x_split"], y_split=t[f"ys{j}"], y_split_slope=1.0,
                                                                            no_y=j < 2, out=t[f"y{j}"])) for j in range(3)])
    c.call = call

    def ref(t):
        pre = ops.unsplit(xs).double().cpu()
        for j in range(3):
            want = F.conv1d(pre, ws[j].double(), bs[j].double())
            bounded(f"conv1d_multi gemm {j}", ops.unsplit(t[f"ys{j}"]), want, 3e-5 + 2.0 ** -21 * want.abs())
        bounded("conv1d_multi gemm y", t["y2"], F.conv1d(pre, ws[2].double(), bs[2].double()), 3e-5)
    c.ref = ref
    return c


# ---- one TDNNF layer per call ------------------------------------------------------------------------------------------------------
@row("sat_tdnnf_layer_f32", "f32 / planes", [(1, 3, 80, 128, 1024, 3, 0, 0.0), (3, 3, 256, 64, 256, 33, 0, 0.66), (1, 1, 256, 64, 256, 32, 1, 0.66),
                                             (3, 3, 1024, 128, 1024, 258, 1, 0.66), (3, 2, 64, 40, 64, 130, 0, 0.66), (3, 3, 256, 64, 256, 295, 2, 0.66)])
def _(B, ctx, feat, bott, out, T, how, bypass):
    """how: 0 = exact f32, 1 = split planes (x f32 for the bypass, y f32 + planes), 2 = planes only (x = NULL, y = NULL)"""
    lib, ops, _ = _sat()
    c = Case()
    mode = 0 if how == 0 else 1
    # the last launch is linearA, a 1x1 conv over t_q frames: exact f32 on the conv tile; on planes the 128 x 256 ring GEMM where 256-column tiles pad
    # the frames (nearly) no more than 128-column ones, else the 128 x 128 GEMM (the dispatch of sat_conv1d_f32; BatchNorm + ReLU keep it off the walk)
    tq_ = T - (ctx - 1)
    c.family = "conv1d_mfma_kernel" if how == 0 else "gemm_f16x3_ring16_kernel" if -(-tq_ // 256) * 256 * 8 <= -(-tq_ // 128) * 128 * 9 else "conv1d_f16x3_k1_kernel"
    x = rand(B, feat, T, seed=T).relu()
    wB, wA = rand(bott, feat, ctx, seed=1, scale=(feat * ctx) ** -0.5), rand(out, bott, 1, seed=2, scale=bott ** -0.5)
    bB, bA = rand(bott, seed=3, scale=0.1), rand(out, seed=4, scale=0.1)
    var = rand(out, seed=6).abs() + 0.5
    scale, shift = 1.0 / torch.sqrt(var + 1e-5), -rand(out, seed=5, scale=0.1) / torch.sqrt(var + 1e-5)
    t_q = T - (ctx - 1)
    pB, aB = _pack(wB, mode)
    pA, aA = _pack(wA, mode)
    planes = how > 0
    xs = ops.act_split(x.to(DEV), 1.0) if planes else None
    if how < 2:
        c.inp("x", x)
    if planes:
        c.inp("x_split", xs)
        c.ws("z_split", B * bott * t_q * 4)             # the bottleneck: scratch, planes only
        c.out("y_split", (B, out // 16, 2, 2, t_q, 8), F16)
    else:
        c.ws("z", B * bott * t_q * 4)
    for n, v in (("wB", pB), ("wA", pA), ("bB", bB), ("bA", bA), ("bn_scale", scale), ("bn_shift", shift)):
        c.inp(n, v)
    if how < 2:
        c.out("y", (B, out, t_q))

    def call(t):
        d = lib.TdnnfLayerDesc()
        d.B, d.feat_dim, d.bottleneck_dim, d.out_dim, d.T_in, d.context_len = B, feat, bott, out, T, ctx
        d.mode, d.bypass_scale = mode, bypass
        d.wB_descale, d.wA_descale = aB.get("w_descale", 1.0), aA.get("w_descale", 1.0)
        d.x, d.x_split, d.wB_packed, d.wA_packed = P(t.get("x")), P(t.get("x_split")), P(t["wB"]), P(t["wA"])
        d.bB, d.bA, d.bn_scale, d.bn_shift = P(t["bB"]), P(t["bA"]), P(t["bn_scale"]), P(t["bn_shift"])
        d.y, d.y_split, d.z, d.z_split = P(t.get("y")), P(t.get("y_split")), P(t.get("z")), P(t.get("z_split"))
        _ok(_L().sat_tdnnf_layer_f32(C.byref(d), _stream()), "sat_tdnnf_layer_f32")
    c.call = call

    def ref(t):          # tests/test_hip_parity.py::test_tdnnf_layer_call_equals_its_two_launches: relative RMS 2e-6 (f32) / 5e-6 (planes)
        from conftest import rms
        xd = x.double()
        lidx = 1 if ctx == 2 else ctx // 2
        v = F.conv1d(F.conv1d(xd, wB.double(), bB.double()), wA.double(), bA.double())
        if bypass:
            v = v + bypass * xd[:, :, lidx:lidx + t_q]
        v = F.relu(v * scale.double()[None, :, None] + shift.double()[None, :, None])
        got = t["y"] if how < 2 else ops.unsplit(t["y_split"])
        err = rms(got.double().cpu().numpy() - v.numpy()) / rms(v.numpy())
        print(f"tdnnf_layer: relative rms error {err:.3e}")
        assert err < (2e-6 if mode == 0 else 5e-6), err
        if how == 1:
            assert torch.equal(t["y_split"], ops.act_split(t["y"].contiguous(), 1.0))
    c.ref = ref
    return c


# ---- fused ResBlock steps, the MRF block, the thin upsamplers (pair.hip, pair32s.hip, pair64.hip, mrf.hip, ups2.hip) -----------
def pair_case(B, T, Cc, k, dil, *, planes, scaled=True, no_y=False, accum=False, family=None, options=(), bound=2e-5, x=None, acc0=None):
    """out = conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 + x.  `bound`: 2e-5 for the general fused steps (tests/test_hip_parity.py::
    test_fused_resblock_pair_matches_torch), 1e-5 for the streaming ones and C = 64 (::test_streaming_resblock_step_matches_the_general_fused_step).
    `x`, `acc0`: a given input and accumulator (a sub-batch or a crop of another case's) in place of the seeded ones"""
    entry = "sat_resblock_pair_scaled_f16x3" if scaled else "sat_resblock_pair_f16x3"
    lib, ops, packing = _sat()
    c = Case(family=family, options=tuple(options))
    x = rand(B, Cc, T, seed=T + Cc) if x is None else x
    w1, w2 = rand(Cc, Cc, k, seed=2, scale=0.6 / np.sqrt(Cc * k)), rand(Cc, Cc, k, seed=3, scale=0.6 / np.sqrt(Cc * k))
    b1, b2 = rand(Cc, seed=4, scale=0.1), rand(Cc, seed=5, scale=0.1)
    acc0 = rand(B, Cc, T, seed=6) if acc0 is None else acc0
    c.data.update(x=x, acc0=acc0)
    p1, p2 = (packing.pack_conv_weight_f16x3(w.to(DEV), scale=scaled) for w in (w1, w2))
    xs = ops.act_split(x.to(DEV), 0.1) if planes else None
    if planes:
        c.inp("x_split", xs)
        c.out("y_split", (B, Cc // 16, 2, 2, T, 8), F16)
    else:
        c.inp("x", x)
    for n, v in (("w1", p1), ("w2", p2), ("b1", b1), ("b2", b2)):
        c.inp(n, v)
    if no_y:
        c.untouched("y", (B, Cc, T))
    elif accum:
        c.inout("y", acc0)
    else:
        c.out("y", (B, Cc, T))

    def call(t):
        d = lib.ConvDesc()
        d.B, d.C_in, d.T_in, d.C_out, d.T_q = B, Cc, T, Cc, T
        d.ksize, d.dilation, d.stride, d.pad_left, d.groups, d.up, d.mode = k, dil, 1, 0, 1, 1, 1
        d.in_lrelu, d.in_slope = 1, 0.1
        d.accum, d.accum_div = int(accum), 3.0 if accum else 0.0
        d.res_scale, d.res_toff, d.res_tstride = 1.0, 0, 1
        d.x_bstride = d.y_bstride = d.res_bstride = Cc * T
        d.x_cstride = d.y_cstride = d.res_cstride = T
        d.bias, d.res = P(t["b2"]), P(t.get("x"))
        d.x_split, d.y_split, d.y_split_slope = P(t.get("x_split")), P(t.get("y_split")), 0.1
        if planes:
            d.res_split, d.res_split_slope = P(t["x_split"]), 0.1
        d.no_y = int(no_y)
        d.w_descale = p2.w_descale
        if scaled:
            _ok(_L().sat_resblock_pair_scaled_f16x3(C.byref(d), P(t.get("x")), P(t["w1"]), P(t["b1"]), p1.w_descale, P(t["w2"]), P(t["y"]), _stream()), entry)
        else:
            _ok(_L().sat_resblock_pair_f16x3(C.byref(d), P(t.get("x")), P(t["w1"]), P(t["b1"]), P(t["w2"]), P(t["y"]), _stream()), entry)
    c.call = call

    def ref(t):
        xd = x.double()
        t1 = F.conv1d(F.leaky_relu(xd, 0.1), w1.double(), b1.double(), dilation=dil, padding=(k * dil - dil) // 2)
        v = F.conv1d(F.leaky_relu(t1, 0.1), w2.double(), b2.double(), padding=(k - 1) // 2) + xd
        if accum:
            v = (acc0.double() + v) / 3
        if not no_y:
            bounded("resblock_pair y", t["y"], v, bound)
        if planes:
            want = F.leaky_relu(v, 0.1)
            bounded("resblock_pair y_split", ops.unsplit(t["y_split"]), want, bound + 2.0 ** -21 * want.abs())
            if not no_y:
                assert torch.equal(t["y_split"], ops.act_split(t["y"].contiguous(), 0.1))
    c.ref = ref
    return c


def pair_rows(name, tile, family, Cc, k, dil, *, scaled=True, extra=(), **kw):
    @row("sat_resblock_pair_scaled_f16x3" if scaled else "sat_resblock_pair_f16x3", name, times(tile) + list(extra))
    def _(B, T):
        return pair_case(B, T, Cc, k, dil, scaled=scaled, family=family, **kw)


pair_rows("C16 f32-in k3", 224, "resblock_pair_f16x3_kernel", 16, 3, 1, planes=False)
pair_rows("C16 f32-in k7 accum", 224, "resblock_pair_f16x3_kernel", 16, 7, 3, planes=False, accum=True)
pair_rows("C32 f32-in k11 unscaled entry", 224, "resblock_pair_f16x3_kernel", 32, 11, 5, planes=False, scaled=False)
pair_rows("C16 planes k7", 224, "resblock_pair16_kernel", 16, 7, 3, planes=True, extra=[(3, 1061)])
pair_rows("C16 planes k11 planes only", 224, "resblock_pair16_kernel", 16, 11, 5, planes=True, no_y=True)
pair_rows("C32 planes k3 streaming", 240, "pair32s_kernel", 32, 3, 5, planes=True, bound=1e-5)
pair_rows("C32 planes k3 streaming 4 waves accum", 112, "pair32s_kernel", 32, 3, 1, planes=True, accum=True, options=(("pair32s_waves", 4, 8),), bound=1e-5)
pair_rows("C32 planes k7 wave-specialised planes only", 240, "pairw_kernel", 32, 7, 3, planes=True, no_y=True, bound=1e-5)
pair_rows("C32 planes k11 wave-specialised planes only", 240, "pairw_kernel", 32, 11, 5, planes=True, no_y=True, bound=1e-5)
pair_rows("C32 planes k3 general step", 224, "resblock_pair32_kernel", 32, 3, 5, planes=True, options=(("pair32s", 0, 1),))
pair_rows("C64 planes k3", 126, "resblock_pair64_kernel", 64, 3, 5, planes=True, bound=1e-5)
pair_rows("C64 planes k7 accum untrimmed halo", 122, "resblock_pair64_kernel", 64, 7, 3, planes=True, accum=True, options=(("trim_halo", 0, 1),), bound=1e-5)
pair_rows("C64 planes k3 wave-specialised", 112, "pairw_kernel", 64, 3, 3, planes=True, options=(("pair64w", 1, 0),), bound=1e-5)


def _mrf_weights(Cc, ks, seed):
    steps = []
    for i in range(3):
        s = seed + 10 * i
        steps.append((rand(Cc, Cc, ks, seed=s, scale=0.7 / np.sqrt(Cc * ks)), rand(Cc, seed=s + 1, scale=0.1),
                      rand(Cc, Cc, ks, seed=s + 2, scale=0.7 / np.sqrt(Cc * ks)), rand(Cc, seed=s + 3, scale=0.1)))
    return steps


def mrf_case(B, T, nb=3, rfp=1, x=None):
    """the C = 16 MRF block in one launch; `x`: a given input in place of the seeded one"""
    lib, ops, packing = _sat()
    Cc = 16
    c = Case(family="mrf16_kernel")
    x = rand(B, Cc, T, seed=T) if x is None else x
    c.data["x"] = x
    xs = ops.act_split(x.to(DEV), 0.1)
    branches = [(3, _mrf_weights(Cc, 3, 100)), (7, _mrf_weights(Cc, 7, 200)), (11, _mrf_weights(Cc, 11, 300))][:nb] if nb == 3 else [(7, _mrf_weights(Cc, 7, 200))]
    desc = {}
    c.inp("x_split", xs)
    for j, (k, steps) in enumerate(branches):
        for i, (w1, b1, w2, b2) in enumerate(steps):
            for h, (w, b) in enumerate(((w1, b1), (w2, b2))):
                wp = packing.pack_conv_weight_f16x3(w.to(DEV))
                desc[(j, i, h)] = wp.w_descale
                c.inp(f"w{j}{i}{h}", wp)
                c.inp(f"b{j}{i}{h}", b)
    ks = lib.int_array([k for k, _ in branches])
    nscratch = _L().sat_resblock_mrf_scratch_bytes(len(branches), ks)
    c.ws("scratch", nscratch)
    c.out("y", (B, Cc, T))
    if nb == 3:
        c.out("y_split", (B, 1, 2, 2, T, 8), F16)

    def call(t):
        d = lib.MrfDesc()
        d.B, d.C, d.T, d.n_branches = B, Cc, T, len(branches)
        for j, (k, steps) in enumerate(branches):
            d.ksize[j] = k
            for i in range(3):
                d.dilation[j][i] = 2 * i + 1
                for h in range(2):
                    d.w[j][i][h], d.bias[j][i][h], d.w_descale[j][i][h] = P(t[f"w{j}{i}{h}"]), P(t[f"b{j}{i}{h}"]), desc[(j, i, h)]
        d.slope, d.x_split = 0.1, P(t["x_split"])
        d.y, d.y_split, d.y_split_slope, d.out_div = P(t["y"]), P(t.get("y_split")), 0.1, 3.0 if nb == 3 else 0.0
        d.residual_from_planes = rfp
        d.scratch, d.scratch_bytes = P(t["scratch"]), nscratch
        _ok(_L().sat_resblock_mrf_f16x3(C.byref(d), _stream()), "sat_resblock_mrf_f16x3")
    c.call = call

    def ref(t):          # tests/test_hip_parity.py::test_fused_mrf_block_c16_equals_the_nine_launch_path: 2e-5 against float64
        xd = ops.unsplit(xs).double().cpu()
        xd = torch.where(xd > 0, xd, xd * 10.0)
        tot = 0
        for k, steps in branches:
            v = xd
            for i, (w1, b1, w2, b2) in enumerate(steps):
                dd = 2 * i + 1
                t1 = F.conv1d(F.leaky_relu(v, 0.1), w1.double(), b1.double(), dilation=dd, padding=dd * (k - 1) // 2)
                v = v + F.conv1d(F.leaky_relu(t1, 0.1), w2.double(), b2.double(), padding=(k - 1) // 2)
            tot = tot + v
        want = tot / 3 if nb == 3 else tot
        bounded("resblock_mrf", t["y"], want, 2e-5)
        if nb == 3:
            assert torch.equal(t["y_split"], ops.act_split(t["y"].contiguous(), 0.1))
    c.ref = ref
    return c


row("sat_resblock_mrf_f16x3", "C16 block", [(b, t, 3, 1) for b, t in times(512)] + [(3, 60, 3, 0), (1, 11, 1, 1), (3, 513, 1, 0)])(mrf_case)


def ups2_case(B, T, cin, x=None):
    """the thin stride-2 upsampler; `x`: a given input in place of the seeded one"""
    _, ops, packing = _sat()
    c = Case(family="ups2_kernel")
    cout = cin // 2
    x = rand(B, cin, T, seed=T + cin) if x is None else x
    c.data["x"] = x
    w, b = rand(cin, cout, 4, seed=2, scale=0.8 / np.sqrt(cin * 2)), rand(cout, seed=3, scale=0.1)
    wc, kp, pl = packing.convtranspose_as_phase_conv(w.to(DEV), 2, 1)
    wp = packing.pack_conv_weight_f16x3(wc, up=2)
    c.inp("x_split", ops.act_split(x.to(DEV), 0.1))
    c.inp("w", wp)
    c.inp("bias", b)
    c.out("y_split", (B, cout // 16, 2, 2, 2 * T, 8), F16)
    c.call = lambda t: ops.upsample2(t["x_split"], _attrs(t["w"], {"w_descale": wp.w_descale}), t["bias"], B, cin, T, y_split_slope=0.1, y_split=t["y_split"])

    def ref(t):      # tests/test_hip_parity.py::test_streaming_upsampler_matches_the_polyphase_conv_and_torch: 1e-5
        want = F.leaky_relu(F.conv_transpose1d(F.leaky_relu(x.double(), 0.1), w.double(), b.double(), stride=2, padding=1), 0.1)
        bounded("upsample2", ops.unsplit(t["y_split"]), want, 1e-5)
    c.ref = ref
    return c


def ups2_rows(cin, tile):
    @row("sat_upsample2_f16x3", f"C{cin}", times(tile))
    def _(B, T):
        return ups2_case(B, T, cin)


ups2_rows(32, 496)
ups2_rows(64, 240)


@row("sat_act_split_f32", "both formats", [(b, 32, t, f) for f in (0, 1) for b, t in times(256)] + [(3, 512, 37, 0)])
def _(B, Cc, T, fmt):
    _, ops, _ = _sat()
    c = Case()
    x = rand(B, Cc, T, seed=T, scale=3.0)
    c.inp("x", x)
    c.out("x_split", (B, Cc // 16, 2, 2, T, 8), F16)
    c.call = lambda t: ops.act_split(t["x"], 0.1, out=t["x_split"], fmt=fmt)

    def ref(t):          # tests/test_hip_parity.py::test_act_split_planes: |hi + lo - lrelu(x)| <= 2^-20 max |lrelu(x)|, and per element what the
        # format gives (include/satools_hip.h): hi and lo are both f16 truncated toward zero, so hi + lo carries 22 significand bits — short of
        # x * slope by less than 2^-21 of it, or by less than 2^-24, the spacing of the f16 subnormals, where lo is one (|x * slope| < 2^-4) —
        # plus one f32 rounding each (2^-24) for the kernel's x * slope and for unsplit's hi + lo.  The slope is the f32 the C ABI passes
        want = F.leaky_relu(x.double(), float(np.float32(0.1)))
        s = t["x_split"]
        if fmt == 0:
            bounded("act_split", ops.unsplit(s), want, 2.0 ** -20 * float(want.abs().max()))
            bounded("act_split", ops.unsplit(s), want, (2.0 ** -21 + 2.0 ** -23) * want.abs() + 2.0 ** -24)
        hi = ops.unsplit(torch.stack([s[:, :, 0], torch.zeros_like(s[:, :, 0])], 2))
        bounded("act_split hi", hi, want, 2.0 ** -10 * want.abs() + 2.0 ** -24)
    c.ref = ref
    return c


@row("sat_planes_f8_sidecar", "e5m2", [(b, 32, t) for b, t in times(256)] + [(3, 256, 77)])
def _(B, Cc, T):
    _, ops, _ = _sat()
    c = Case()
    x = rand(B, Cc, T, seed=T, scale=3.0)
    x[0, :, :1] *= 300.0
    xs = ops.act_split(x.to(DEV), 0.1)
    c.inp("x_split", xs)
    c.out("x_split8", (B, Cc // 16, 2, T, 16), U8)
    c.call = lambda t: ops.planes_f8_sidecar(t["x_split"], out=t["x_split8"])

    def ref(t):          # tests/test_hip_f8r.py::test_planes_f8_sidecar_is_e5m2_of_the_plane_values: bit for bit
        import test_hip_f8r as f8
        hi, lo = f8._planes_hi_lo(ops, xs)
        assert torch.equal(t["x_split8"].cpu(), f8._sidecar_bytes(hi, lo))
    c.ref = ref
    return c


# ---- the generator (csrc/hifigan.hip) --------------------------------------------------------------------------------------------
@row("sat_hifigan_convpost_f32", "both forms", [(1, 16, 2, 1), (3, 16, 1022, 1), (1, 32, 1023, 0), (3, 16, 1024, 1), (3, 32, 2085, 0), (3, 16, 2085, 1),
                                                  (3, 39, 1025, 0)])
def _(B, Cc, T, quad):          # POST_TILE = 1024 of the T + 1 outputs per block; C = 39 = POST_MAXC: the widest [C][1030] tile that fits the LDS
    c = Case(options=(("convpost_quad", quad, 1),))
    # weights of 0.1 at C = 16 as in the existing test, 16 / C of that at other C: the rounding of an f32 sum grows with the number of its terms times
    # the size of its partial sums (~ sqrt(C) |w|), so this keeps it where the 2e-6 below was set
    x, w, b = rand(B, Cc, T, seed=T), rand(Cc, 7, seed=2, scale=0.1 * 16 / Cc), rand(1, seed=3, scale=0.1)
    c.inp("x", x)
    c.inp("w", w)
    c.inp("bias", b)
    c.out("y", (B, 1, T + 1))
    c.call = lambda t: _ok(_L().sat_hifigan_convpost_f32(P(t["x"]), P(t["w"]), P(t["bias"]), P(t["y"]), B, Cc, T, _stream()), "sat_hifigan_convpost_f32")
    # tests/test_hip_parity.py::test_convpost_matches_oracle: 2e-6
    c.ref = lambda t: bounded("convpost", t["y"], torch.tanh(F.conv1d(F.pad(F.leaky_relu(x.double()), (1, 0), mode="reflect"), w.double().unsqueeze(0), b.double(),
                                                                    padding=3)), 2e-6)
    return c


_GEN = {}


def _generator(precision):
    """the synthetic fbank-tag generator with its packed weights installed in a handle of its own, one per arithmetic"""
    if precision not in _GEN:
        import satools_amd
        m = satools_amd.load_model("synthetic:hifigan_bn_tdnnf_600h_vq_48_v1")
        m.to(DEV)
        g = m.hifigan
        g.precision = precision
        g.invalidate()
        g._prepare(torch.device(DEV))
        _GEN[precision] = (m, g)
    return _GEN[precision][1]


@row("sat_hifigan_forward_f32", "whole generator", [("f32", 1, 7, 0), ("f16x3", 3, 25, 0), ("f16x3", 1, 40, 1), ("f16f8r", 1, 33, 0), ("f16f8r", 3, 25, 1),
                                                         ("f16f8r", 27, 250, 0)])
def _(precision, B, T, probe):
    """the small f16f8r shapes force the ring (set_force_f8); 27 x 250 frames reaches it by size, as a production batch does: 8 tiles of 256 x 160 per
    utterance in the first stage, 216 tiles >= three quarters of 256 CUs (convring_wanted) — the one full-size shape here, a kernel selected by size"""
    c = Case()
    forced = precision == "f16f8r" and B < 27
    g = _generator(precision)
    up = int(np.prod(g.upsample_rates))
    x = rand(B, g.imput_dim, T, seed=T)
    need = _L().sat_hifigan_workspace_bytes(g._handle, B, T)
    c.inp("x", x)
    c.out("y", (B, 1, T * up + 1))
    c.ws("ws", need)
    if probe:
        c.inout("probe", torch.zeros(2 * len(g.upsample_rates), dtype=I64))

    def call(t):
        g.set_force_f8(int(forced))          # a batch this small is below the ring kernel's default dispatch
        _ok(_L().sat_hifigan_set_range_probe(g._handle, P(t.get("probe"))), "sat_hifigan_set_range_probe")
        try:
            _ok(_L().sat_hifigan_forward_f32(g._handle, P(t["x"]), P(t["y"]), P(t["ws"]), need, B, T, _stream()), "sat_hifigan_forward_f32")
            torch.cuda.synchronize()
        finally:
            _ok(_L().sat_hifigan_set_range_probe(g._handle, None), "sat_hifigan_set_range_probe")
            g.set_force_f8(0)
        ran = g.last_arithmetic
        assert ran.startswith(precision), (ran, precision)          # "f16f8r(stages ...)": the ring ran with 8-bit cross terms
    c.call = call

    def ref(t):          # a whole pipeline: the plain call is its reference (property E)
        assert bool(torch.isfinite(t["y"]).all()) and float(t["y"].abs().max()) <= 1.0
        if probe:
            assert int(t["probe"][0::2].sum()) == 0
    c.ref = ref
    return c


# ---- the tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("p", [(r, s) for r in ROWS for s in r.shapes], ids=_id)
def test_no_access_outside_the_buffers(p):
    r, shape = p
    case = r.make(*shape)
    lib = _sat()[0]

    def call(t):
        case.call(t)
        full = lib.lib().sat_last_dispatch_name().decode()
        name = full.split("<")[0].strip()          # (the launcher's template arguments; "layernorm_ch_kernel<conv0>" is a name of its own)
        SEEN.update((name, full))
        if case.family is not None:
            assert name == case.family, f"meant to hit {case.family}, the dispatch picked {name}"

    with _options(case.options):
        v, m, plain = run_case(case.specs, call, DEV, tol=case.tol, sync=torch.cuda.synchronize)
    assert not v, f"{r.entry} [{r.name}] {shape}:\n" + "\n".join(str(x) for x in v)
    if case.ref is not None:
        case.ref(m.t)


@pytest.mark.gpu
def test_convpost_refuses_more_channels_than_fit_the_lds():
    """found by this table: the entry took C up to 64, but a block keeps C x (1030 + 7) floats in LDS, and past C = 39 that is more than the
    160 KiB a block can have — the call came back as a HIP error from the attribute call, not as a refusal.  Now: SAT_ERR_INVALID before
    anything is asked of the runtime, and the next call works"""
    x, w, b = rand(1, 40, 64).to(DEV), rand(40, 7, seed=2, scale=0.04).to(DEV), rand(1, seed=3, scale=0.1).to(DEV)
    y = torch.full((1, 1, 65), 7.0, device=DEV)
    assert _L().sat_hifigan_convpost_f32(P(x), P(w), P(b), P(y), 1, 40, 64, _stream()) == -1
    assert b"C=40" in _L().sat_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    _ok(_L().sat_hifigan_convpost_f32(P(x), P(w), P(b), P(y), 1, 39, 64, _stream()), "sat_hifigan_convpost_f32")
    want = torch.tanh(F.conv1d(F.pad(F.leaky_relu(x[:, :39].cpu().double()), (1, 0), mode="reflect"), w[:39].cpu().double().unsqueeze(0), b.cpu().double(), padding=3))
    bounded("convpost", y, want, 2e-6)          # tests/test_hip_parity.py::test_convpost_matches_oracle


@pytest.mark.gpu
def test_every_dispatch_family_was_seen():
    """runs after the table (file order): every kernel family a conv-shaped entry point can dispatch to was hit by a row that meant to"""
    missing = [f for f in FAMILIES if f not in SEEN]
    assert not missing, f"kernel families no row of the table reached: {missing}"
