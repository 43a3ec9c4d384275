"""Thin Python wrappers over the C ABI (tensor checks + descriptor filling).
All tensors are f32, channel-major [B, C, T], on the HIP device."""
import ctypes as C

import torch

from . import _lib
from ._lib import ConvDesc, check, lib, ptr, stream


def _f32c(t):
    if t.dtype != torch.float32:
        raise _lib.SatError(f"expected float32 tensor, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _descale(w_packed, mode=1):
    """power-of-two layer scale of split-f16 packed weights (packing.pack_conv_weight_f16x3 attaches it as `.w_descale`).
    The attribute does not survive .to() / .clone() / .contiguous() / indexing: a packed tensor WITHOUT it in split-f16 mode is
    refused instead of being multiplied as if its scale were 1 (every output of the layer would be off by 2^e)."""
    if int(mode) not in (1, 3):
        return float(getattr(w_packed, "w_descale", 1.0))
    d = getattr(w_packed, "w_descale", None)
    if d is None:
        raise _lib.SatError("split-f16 packed weights without .w_descale: pack on the target device (packing.pack_conv_weight_f16x3), "
                            "move them with packing.move_packed(), or set w.w_descale = 1.0 for weights packed with scale=False")
    return float(d)


def _strided3(t):
    """[B, C, T] tensor usable by the conv kernel: f32, innermost axis contiguous (views with a row
    pitch are fine: the kernel takes batch / channel strides)"""
    if t.dtype != torch.float32:
        raise _lib.SatError(f"expected float32 tensor, got {t.dtype}")
    return t if t.stride(-1) == 1 else t.contiguous()


def conv1d(x, w_packed, c_out, ksize, **kw):
    """Fused conv (see include/satools_hip.h sat_conv1d_f32); keyword arguments: `_conv1d_desc`."""
    d, x, out, keep = _conv1d_desc(x, w_packed, c_out, ksize, **kw)
    check(lib().sat_conv1d_f32(C.byref(d), ptr(x, strided=True), ptr(w_packed), ptr(out, strided=True), stream()),
          "sat_conv1d_f32")
    return out


def conv1d_multi(jobs):
    """`jobs` = 1..3 tuples (x, w_packed, c_out, ksize, kwargs) as for `conv1d`, independent of each other (or coupled only
    through `accum` on one `out` in list order): sat_conv1d_multi_f32 — one launch of the LDS-DMA ring kernel where it
    serves them all, else the single calls in order.  Returns the list of outputs."""
    n = len(jobs)
    descs = (ConvDesc * n)()
    xs, ws, ys, outs, keep = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)(), [], []
    for j, (x, w, c_out, ksize, kw) in enumerate(jobs):
        d, x, out, k = _conv1d_desc(x, w, c_out, ksize, **kw)
        descs[j] = d
        xs[j], ws[j], ys[j] = ptr(x, strided=True), ptr(w), ptr(out, strided=True)
        outs.append(out)
        keep.append((x, k))
    check(lib().sat_conv1d_multi_f32(descs, xs, ws, ys, n, stream()), "sat_conv1d_multi_f32")
    return outs


def _conv1d_desc(x, w_packed, c_out, ksize, *, bias=None, dilation=1, stride=1, pad_left=0, pad_right=None, groups=1,
                 up=1, in_lrelu=None, res=None, res_scale=1.0, res_toff=0, res_tstride=1, ch_scale=None, ch_shift=None,
                 relu=False, gelu=False, post_res=None, out=None, accum=False, accum_div=0.0, mode=0, t_out=None,
                 x_split=None, y_split=None, y_split_slope=1.0, no_y=False, y_split_format=0, res_split=None,
                 res_split_slope=1.0, relu_first=False, x_wrap_channels=0, c_in=None, up_grouped=False, up_zero_taps=0,
                 x_split8=None, y_split8=None, y_split_hi_only=False):
    """Descriptor of a fused conv (see include/satools_hip.h sat_conv1d_f32).  `pad_right` defaults to the
    'same'-style value implied by pad_left for stride 1; T_q is derived like torch does:
    T_q = (T_in + pad_left + pad_right - dilation*(ksize-1) - 1)//stride + 1 (`t_out` caps it).
    `post_res` is a residual added AFTER the activation (y = post_res + act(conv(x))).
    Split planes (mode=CONV_F16X3): `x_split` = act_split(pre(x)) replaces the staging of x (x then only
    gives the shape); `y_split` (a split_like buffer) also receives split(lrelu(y, y_split_slope));
    `no_y` skips the f32 store; `res_split` takes the residual from SPLIT_F16 planes of lrelu(r, res_split_slope).
    `x_wrap_channels` = Cw (1x1 conv on split planes): the planes hold Cw channels and the weight's input channels
    c >= Cw read channel c - Cw one position later (sat_conv1d_desc.x_wrap_channels); `x` gives [B, Cw, T] and
    `c_in` the weight's input channels.  `up_grouped` (up = 4, planes in and out): the polyphase weight's rows are ordered (16-channel
    group, phase, channel) — packing.convtranspose_as_phase_conv(..., grouped=True) — and `up_zero_taps` names its all-zero (tap slot,
    phase) pairs (packing.convtranspose_zero_taps), sat_conv1d_desc.up_grouped / up_zero_taps.
    mode=CONV_F16F8R (the LDS-DMA ring kernel with e4m3 cross terms; weights from packing.pack_conv_weight_f16f8r): `x_split8` = the
    e4m3 sidecar of x_split (planes_f8_sidecar, or a producer's `y_split8`); `y_split8` (a sidecar_like buffer) receives the sidecar of
    y_split; `y_split_hi_only` leaves the lo units of y_split unwritten."""
    x = _strided3(x)
    c_in_w = c_in
    B, c_in, t_in = x.shape
    if pad_right is None:
        pad_right = dilation * (ksize - 1) - pad_left if up == 1 and stride == 1 else 0
    if up > 1:
        t_q = t_in
    else:
        t_q = (t_in + pad_left + pad_right - dilation * (ksize - 1) - 1) // stride + 1
    if t_out is not None:
        t_q = min(t_q, int(t_out))
    if t_q <= 0:
        raise _lib.SatError("conv1d: input too short for this kernel")
    if out is None:
        out = torch.empty(B, c_out, t_q * up, dtype=torch.float32, device=x.device)
    if post_res is not None:
        assert res is None
        res = post_res
    d = ConvDesc()
    d.B, d.C_in, d.T_in, d.C_out, d.T_q = B, (c_in if c_in_w is None else int(c_in_w)), t_in, c_out, t_q
    d.ksize, d.dilation, d.stride, d.pad_left, d.groups, d.up = ksize, dilation, stride, pad_left, groups, up
    d.mode = int(mode)
    d.w_descale = _descale(w_packed, mode)      # power-of-two layer scale of split-f16 packed weights (packing.py)
    d.in_lrelu = 0 if in_lrelu is None else 1
    d.in_slope = 0.0 if in_lrelu is None else float(in_lrelu)
    d.relu, d.gelu, d.res_after_act = int(relu), int(gelu), int(post_res is not None)
    d.accum = int(accum)
    d.accum_div = float(accum_div)
    d.res_scale, d.res_toff, d.res_tstride = float(res_scale), int(res_toff), int(res_tstride)
    d.x_bstride, d.x_cstride = x.stride(0), x.stride(1)
    d.y_bstride, d.y_cstride = out.stride(0), out.stride(1)
    if res is not None:
        res = _strided3(res)
        d.res_bstride, d.res_cstride = res.stride(0), res.stride(1)
    d.bias = ptr(bias)
    d.res = ptr(res, strided=True)
    d.ch_scale = ptr(ch_scale)
    d.ch_shift = ptr(ch_shift)
    d.x_split, d.y_split = ptr(x_split), ptr(y_split)
    d.y_split_slope, d.no_y, d.y_split_format = float(y_split_slope), int(no_y), int(y_split_format)
    d.res_split, d.res_split_slope = ptr(res_split), float(res_split_slope)
    d.relu_first = int(relu_first)
    d.x_wrap_channels = int(x_wrap_channels)
    if up_grouped and up_zero_taps:
        # the mask is a promise about the WEIGHTS (the kernel leaves those products out): only zeros the packer saw may be claimed
        have = getattr(w_packed, "up_zero_taps", None)
        if have is None or (int(up_zero_taps) & ~int(have)):
            raise _lib.SatError(f"conv1d: up_zero_taps = {int(up_zero_taps):#x} claims all-zero (tap slot, phase) pairs the packed weights do not have "
                                f"({'no record on the packed tensor' if have is None else hex(int(have))}: pack with packing.pack_conv_weight_f16x3(..., up=4) "
                                "from packing.convtranspose_as_phase_conv(..., grouped=True))")
    d.up_grouped, d.up_zero_taps = int(bool(up_grouped)), int(up_zero_taps)
    if int(mode) == _lib.CONV_F16F8R:
        # the ring kernel moves these buffers by LDS-DMA at offsets derived from the SHAPES: a packing of the other kind (half the
        # bytes) or a short sidecar would be read / written past its end, not refused (round-5 advisor item)
        ci = int(d.C_in)
        nq = (-(-ci // 32) * ksize + 1) // 2
        co_pad = -(-c_out // 64) * 64
        want = 2 * nq * 8 * co_pad * 16
        if w_packed.dtype != torch.uint8 or w_packed.numel() != want:
            raise _lib.SatError(f"conv1d(f16f8r): w_packed must be the packing of packing.pack_conv_weight_f16f8r for [{c_out}, {ci}, {ksize}] "
                                f"({want} bytes of uint8), got {w_packed.numel()} elements of {w_packed.dtype}")
        if x_split is None or x_split.numel() * x_split.element_size() < B * ci * t_in * 4:
            raise _lib.SatError(f"conv1d(f16f8r): x_split must hold the planes of [{B}, {ci}, {t_in}] ({B * ci * t_in * 4} bytes)")
        if x_split8 is None or x_split8.numel() * x_split8.element_size() < B * ci * t_in * 2:
            raise _lib.SatError(f"conv1d(f16f8r): x_split8 must hold the sidecar of [{B}, {ci}, {t_in}] ({B * ci * t_in * 2} bytes: ops.sidecar_like)")
    if y_split8 is not None and y_split8.numel() * y_split8.element_size() < B * c_out * t_q * up * 2:
        raise _lib.SatError(f"conv1d: y_split8 must hold the sidecar of [{B}, {c_out}, {t_q * up}] ({B * c_out * t_q * up * 2} bytes: ops.sidecar_like)")
    d.x_split8, d.y_split8, d.y_split_hi_only = ptr(x_split8), ptr(y_split8), int(bool(y_split_hi_only))
    return d, x, out, res      # (res: the possibly re-laid-out residual must outlive the launch)


def tdnnf_layer(x, wB, bB, wA, bA, bottleneck_dim, out_dim, context_len, *, bn_scale=None, bn_shift=None, bypass_scale=0.0, mode=0,
                x_split=None, y_split=None, z_split=None, no_y=False, bypass_from_planes=False):
    """One TDNNF layer in ONE C-ABI call (sat_tdnnf_layer_f32; chain/nn.py:267-347): linearB over `context_len` frames, linearA, the bypass
    `bypass_scale * x[t + identity_lidx]`, folded BatchNorm, ReLU.  x [B, feat, T_in] f32 -> y [B, out_dim, T_in - context_len + 1];
    on split planes (mode=CONV_F16X3 with `x_split` and a `z_split` scratch) the bottleneck exists only as planes and `y_split`
    also receives the planes of y.  The two launches (and the bits) of the two conv1d calls it replaces.
    On split planes: `no_y` — y is not stored (the returned tensor is an UNINITIALISED shape carrier for a successor that takes `y_split`);
    `bypass_from_planes` — `x` only gives the shape (it may be such a carrier) and the bypass is rebuilt from `x_split` (hi + lo: 22
    significand bits of the input)."""
    on_planes = int(mode) == _lib.CONV_F16X3 and z_split is not None
    no_y = bool(no_y) and on_planes and y_split is not None
    x_unused = bool(bypass_from_planes) and on_planes and x_split is not None
    if bypass_from_planes and not x_unused:
        raise _lib.SatError("tdnnf_layer: bypass_from_planes needs mode=CONV_F16X3 with x_split and z_split")
    x = x if x_unused else _f32c(x)
    B, feat, t_in = x.shape
    t_q = t_in - (int(context_len) - 1)
    if t_q <= 0:
        raise _lib.SatError("tdnnf_layer: input too short for this context")
    y = torch.empty(B, out_dim, t_q, dtype=torch.float32, device=x.device)
    planes = int(mode) == _lib.CONV_F16X3 and z_split is not None
    z = None if planes else torch.empty(B, bottleneck_dim, t_q, dtype=torch.float32, device=x.device)
    d = _lib.TdnnfLayerDesc()
    d.B, d.feat_dim, d.bottleneck_dim, d.out_dim, d.T_in, d.context_len = B, feat, int(bottleneck_dim), int(out_dim), t_in, int(context_len)
    d.mode, d.bypass_scale = int(mode), float(bypass_scale)
    d.wB_descale, d.wA_descale = _descale(wB, mode), _descale(wA, mode)
    d.x, d.x_split, d.wB_packed, d.wA_packed = (None if x_unused else ptr(x)), ptr(x_split), ptr(wB), ptr(wA)
    d.bB, d.bA, d.bn_scale, d.bn_shift = ptr(bB), ptr(bA), ptr(bn_scale), ptr(bn_shift)
    d.y, d.y_split, d.z, d.z_split = (None if no_y else ptr(y)), ptr(y_split), ptr(z), ptr(z_split)
    check(lib().sat_tdnnf_layer_f32(C.byref(d), stream()), "sat_tdnnf_layer_f32")
    return y


def convpost(x, w, bias):
    x = _f32c(x)
    B, c, t = x.shape
    y = torch.empty(B, 1, t + 1, dtype=torch.float32, device=x.device)
    check(lib().sat_hifigan_convpost_f32(ptr(x), ptr(w), ptr(bias), ptr(y), B, c, t, stream()),
          "sat_hifigan_convpost_f32")
    return y


def fbank_cmvn_pad(wav, window, mel, mel_lo, mel_hi, *, scale=32768.0, pad=0, cmvn=True):
    wav = _f32c(wav)
    B, n = wav.shape
    n_mel = mel.shape[0]
    m = (n + 80) // 160
    ws_bytes = lib().sat_fbank_workspace_bytes(B, n)
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.float32, device=wav.device)
    out = torch.empty(B, n_mel, m + 2 * pad, dtype=torch.float32, device=wav.device)
    check(lib().sat_fbank_cmvn_pad_f32(ptr(wav), ptr(out), ptr(window), ptr(mel), ptr(mel_lo), ptr(mel_hi), ptr(ws),
                                       ws_bytes, B, n, float(scale), n_mel, pad, int(cmvn), stream()),
          "sat_fbank_cmvn_pad_f32")
    return out


def vq_tiled(z, codebook, want_dist=False, tie=None):
    """`vq` for codebooks of up to 1024 codes (sat_vq_argmin_gather_tiled_f32 / _tiled_tie_f32: the codebook walked in 64-code tiles
    through LDS); the same arguments and results, for at most 64 codes the same bits"""
    z = _f32c(z)
    codebook = _f32c(codebook)
    B, D, T = z.shape
    n_codes = codebook.shape[0]
    q = torch.empty_like(z)
    idx = torch.empty(B, T, dtype=torch.int32, device=z.device)
    dist = torch.empty(B, T, n_codes, dtype=torch.float32, device=z.device) if want_dist else None
    if tie is not None:
        pair, scale, count = tie
        if (tuple(pair.shape) != (n_codes, n_codes) or pair.dtype != torch.float32 or not pair.is_contiguous() or count.dtype != torch.int32 or
                count.numel() != 3 * B):
            raise _lib.SatError("vq_tiled: tie = (pair_dist [n_codes, n_codes] f32, tie_scale, tie_count [3, B] int32: counts | first | last near-tie frame)")
        check(lib().sat_vq_argmin_gather_tiled_tie_f32(ptr(z), ptr(codebook), ptr(q), ptr(idx), ptr(dist), ptr(pair), float(scale), ptr(count),
                                                       B, D, T, n_codes, stream()), "sat_vq_argmin_gather_tiled_tie_f32")
        return q, idx, dist
    check(lib().sat_vq_argmin_gather_tiled_f32(ptr(z), ptr(codebook), ptr(q), ptr(idx), ptr(dist), B, D, T, n_codes,
                                               stream()), "sat_vq_argmin_gather_tiled_f32")
    return q, idx, dist


def vq(z, codebook, want_dist=False, tie=None):
    """`tie` = (pair_dist [n_codes, n_codes], tie_scale, tie_count [3, B] int32: counts (zeroed) | first (INT32_MAX) | last (-1) near-tie
    frame): also count, per utterance, the frames whose two best codes are a near-tie (sat_vq_argmin_gather_tie_f32)"""
    z = _f32c(z)
    B, D, T = z.shape
    n_codes = codebook.shape[0]
    q = torch.empty_like(z)
    idx = torch.empty(B, T, dtype=torch.int32, device=z.device)
    dist = torch.empty(B, T, n_codes, dtype=torch.float32, device=z.device) if want_dist else None
    if tie is not None:
        pair, scale, count = tie
        if tuple(pair.shape) != (n_codes, n_codes) or pair.dtype != torch.float32 or count.dtype != torch.int32 or count.numel() != 3 * B:
            raise _lib.SatError("vq: tie = (pair_dist [n_codes, n_codes] f32, tie_scale, tie_count [3, B] int32: counts | first | last near-tie frame)")
        check(lib().sat_vq_argmin_gather_tie_f32(ptr(z), ptr(codebook), ptr(q), ptr(idx), ptr(dist), ptr(pair), float(scale), ptr(count),
                                                 B, D, T, n_codes, stream()), "sat_vq_argmin_gather_tie_f32")
        return q, idx, dist
    check(lib().sat_vq_argmin_gather_f32(ptr(z), ptr(codebook), ptr(q), ptr(idx), ptr(dist), B, D, T, n_codes,
                                         stream()), "sat_vq_argmin_gather_f32")
    return q, idx, dist


def pad_replicate(x, left, right, interleave_right=False):
    x = _f32c(x)
    B, c, t = x.shape
    y = torch.empty(B, c, left + t + right, dtype=torch.float32, device=x.device)
    check(lib().sat_pad_replicate_f32(ptr(x), ptr(y), B, c, t, left, right, int(interleave_right), stream()),
          "sat_pad_replicate_f32")
    return y


def f0_norm_transform_(f0, quant_bins=0, noise=None):
    """in place on a contiguous device tensor: batch-coupled mean/var normalisation over the
    non-zero entries, optional quantisation and additive noise"""
    if not f0.is_contiguous():
        raise _lib.SatError("f0 must be contiguous for the in-place normalisation")
    n = f0.numel()
    stats = torch.empty(2, dtype=torch.float32, device=f0.device)
    check(lib().sat_f0_stats_f32(ptr(f0), n, ptr(stats), stream()), "sat_f0_stats_f32")
    if noise is not None:
        noise = _f32c(noise)
        assert noise.numel() == n
    check(lib().sat_f0_apply_f32(ptr(f0), n, ptr(stats), int(quant_bins), ptr(noise), stream()), "sat_f0_apply_f32")
    return f0


def assemble_input(bn, f0, spk_idx, n_spk):
    bn = _f32c(bn)
    f0 = _f32c(f0)
    B, c_bn, T = bn.shape
    t_f0 = f0.shape[-1]
    assert f0.numel() == B * t_f0
    x = torch.empty(B, c_bn + 1 + n_spk, T, dtype=torch.float32, device=bn.device)
    check(lib().sat_assemble_input_f32(ptr(bn), ptr(f0), ptr(spk_idx), ptr(x), B, c_bn, T, t_f0, n_spk, stream()),
          "sat_assemble_input_f32")
    return x


def generator_input(bn, f0, stats, slice_stat=None, quant_bins=0, noise=None, spk=None, want_norm=True):
    """sat_generator_input_f32 (include/satools_hip_geninput.h): -> (x [B, C_bn + 1 + n_spk, T], f0_norm or None), one launch.
    `bn` [B, C_bn, T] f32 with ANY positive strides (the permuted view of an extractor's [B, T, C_bn] goes in as it is); `f0` the raw
    track, [S, R, T_f0] (or [R, T_f0]: S = 1) with S * R = B, not written; `stats` [n_stats, 2] = {mean, std} on the device;
    `slice_stat` a HOST sequence of S ints (rows of `stats`) or None = row 0 for every slice — checked here against n_stats, since a
    wrong entry only makes the kernel skip the slice; `quant_bins` / `noise` ([B, T_f0]) as in sat_f0_apply_f32; `spk` [B, n_spk] f32
    or None.  `f0_norm` holds the normalised values (zeros kept) before quantisation and noise, shaped like `f0`."""
    if bn.dtype != torch.float32 or bn.dim() != 3:
        raise _lib.SatError(f"generator_input: bn must be a float32 [B, C_bn, T] tensor, got {bn.dtype} {tuple(bn.shape)}")
    f0 = _f32c(f0)
    f3 = f0.unsqueeze(0) if f0.dim() == 2 else f0
    if f3.dim() != 3:
        raise _lib.SatError(f"generator_input: f0 must be [S, R, T_f0] or [R, T_f0], got {tuple(f0.shape)}")
    B, c_bn, T = bn.shape
    S, R, t_f0 = f3.shape
    stats = _f32c(stats)
    if stats.dim() != 2 or stats.shape[1] != 2:
        raise _lib.SatError(f"generator_input: stats must be [n_stats, 2], got {tuple(stats.shape)}")
    n_stats = stats.shape[0]
    keep = None
    if slice_stat is not None:
        host = [int(v) for v in (slice_stat.tolist() if torch.is_tensor(slice_stat) else slice_stat)]
        if len(host) != S:
            raise _lib.SatError(f"generator_input: slice_stat has {len(host)} entries for {S} slices")
        for i, v in enumerate(host):
            if not 0 <= v < n_stats:
                raise _lib.SatError(f"generator_input: slice_stat[{i}] = {v} outside 0 .. {n_stats - 1}")
        keep = torch.tensor(host, dtype=torch.int32).pin_memory().to(bn.device, non_blocking=True)
    if noise is not None:
        noise = _f32c(noise)
        if noise.numel() != B * t_f0:
            raise _lib.SatError(f"generator_input: noise has {noise.numel()} elements, f0 rows have {B} x {t_f0}")
    n_spk = 0
    if spk is not None:
        spk = _f32c(spk)
        if spk.dim() != 2 or spk.shape[0] != B:
            raise _lib.SatError(f"generator_input: spk must be [B, n_spk] with B = {B}, got {tuple(spk.shape)}")
        n_spk = spk.shape[1]
        if n_spk == 0:
            spk = None
    for t in (f3, stats, noise, spk):
        if t is not None and t.device != bn.device:
            raise _lib.SatError("generator_input: every tensor on bn's device")
    x = torch.empty(B, c_bn + 1 + n_spk, T, dtype=torch.float32, device=bn.device)
    norm = torch.empty_like(f0) if want_norm else None
    d = _lib.GenInputDesc(B=B, C_bn=c_bn, T=T, T_f0=t_f0, S=S, R=R, n_stats=n_stats, n_spk=n_spk, quant_bins=int(quant_bins), reserved=0,
                          bn_bstride=bn.stride(0), bn_cstride=bn.stride(1), bn_tstride=bn.stride(2),
                          bn=bn.data_ptr() if bn.is_cuda else ptr(bn), f0=ptr(f3), stats=ptr(stats), slice_stat=ptr(keep), noise=ptr(noise),
                          spk=ptr(spk), x=ptr(x), f0_norm=ptr(norm))
    check(lib().sat_generator_input_f32(C.byref(d), stream()), "sat_generator_input_f32")
    return x, norm


def pcm16_to_f32(pcm):
    """int16 PCM on the device -> f32 in [-1, 1): s / 32768, what torchaudio.load hands the reference (utils/kaldi.py:113-125)"""
    if pcm.dtype != torch.int16 or not pcm.is_cuda:
        raise _lib.SatError("pcm16_to_f32: an int16 tensor on the GPU")
    pcm = pcm.contiguous()
    y = torch.empty(pcm.shape, dtype=torch.float32, device=pcm.device)
    if pcm.numel():
        check(lib().sat_pcm16_to_f32(ptr(pcm), ptr(y), pcm.numel(), stream()), "sat_pcm16_to_f32")
    return y


def pcm16_from_f32(x, out=None):
    """f32 waveforms on the device -> the int16 samples torchaudio.save(encoding='PCM_S', bits_per_sample=16) writes (bin/pipeline.py:159):
    round-half-even of x * 32768, clipped"""
    x = _f32c(x)
    if not x.is_cuda:
        raise _lib.SatError("pcm16_from_f32: a tensor on the GPU")
    y = torch.empty(x.shape, dtype=torch.int16, device=x.device) if out is None else out
    if y.dtype != torch.int16 or y.shape != x.shape or not y.is_contiguous() or y.device != x.device:
        raise _lib.SatError("pcm16_from_f32: `out` must be a contiguous int16 tensor of x's shape on x's device")
    if x.numel():
        check(lib().sat_pcm16_from_f32(ptr(x), ptr(y), x.numel(), stream()), "sat_pcm16_from_f32")
    return y


# ---- wav2vec2 support -------------------------------------------------------------------------------
def w2v2_conv0(wav, w, bias, stride=5):
    wav = _f32c(wav)
    B, n = wav.shape
    c, k = w.shape
    t = (n - k) // stride + 1
    y = torch.empty(B, c, t, dtype=torch.float32, device=wav.device)
    check(lib().sat_w2v2_conv0_f32(ptr(wav), ptr(w), ptr(bias), ptr(y), B, n, c, k, stride, stream()), "sat_w2v2_conv0_f32")
    return y


def w2v2_conv0_ln(wav, w, bias, gamma, beta, gelu=True, split_phases=True, planes=True, want_f32=False, stride=5):
    """layernorm_ch(w2v2_conv0(wav, w, bias), gamma, beta, ...) in one kernel (the same bits): returns (y, planes)"""
    wav = _f32c(wav)
    B, n = wav.shape
    c, k = w.shape
    t = (n - k) // stride + 1
    y = torch.empty((B, 2 * c, (t + 1) // 2) if split_phases else (B, c, t), dtype=torch.float32, device=wav.device)
    ys = split_like(B, y.shape[1], y.shape[2], wav.device) if planes else None
    check(lib().sat_w2v2_conv0_layernorm_f32(ptr(wav), ptr(w), ptr(bias), ptr(gamma), ptr(beta), ptr(y) if want_f32 else None,
                                             ptr(ys), B, n, c, k, stride, y.stride(0), y.stride(1), int(gelu), int(split_phases),
                                             stream()), "sat_w2v2_conv0_layernorm_f32")
    return y, ys


def layernorm_ch(x, gamma, beta, gelu=False, split_phases=False, planes=False, want_f32=True):
    """LayerNorm over channels of [B, C, T]; split_phases -> [B, 2C, ceil(T/2)] (even | odd frames).
    planes: also (want_f32=False: only) write the result as split planes for a following split-f16 conv and
    return (y, planes) — without want_f32 `y` is an unwritten tensor that only carries the shape."""
    x = _strided3(x)
    B, c, t = x.shape
    y = torch.empty((B, 2 * c, (t + 1) // 2) if split_phases else (B, c, t), dtype=torch.float32, device=x.device)
    if not planes:
        check(lib().sat_layernorm_channels_f32(ptr(x, strided=True), ptr(gamma), ptr(beta), ptr(y), B, c, t, x.stride(0),
                                               x.stride(1), y.stride(0), y.stride(1), int(gelu), int(split_phases),
                                               stream()), "sat_layernorm_channels_f32")
        return y
    ys = split_like(B, y.shape[1], y.shape[2], x.device)
    check(lib().sat_layernorm_channels_planes_f32(ptr(x, strided=True), ptr(gamma), ptr(beta), ptr(y) if want_f32 else None,
                                                  ptr(ys), B, c, t, x.stride(0), x.stride(1), y.stride(0), y.stride(1),
                                                  int(gelu), int(split_phases), stream()),
          "sat_layernorm_channels_planes_f32")
    return y, ys


def attention_scores(q, k, st, B, heads, hd, T):
    """st[(b,h)*T + j][q] = sum_c k[b][h*hd + c][j] * q[b][h*hd + c][q]: a grouped 1x1 conv whose packed weights
    ARE the [hd][pitch] head slices of k (ci = c, co = j)"""
    pitch = k.shape[2]
    assert k.is_contiguous() and q.is_contiguous() and hd % 16 == 0
    assert pitch == ((T + 63) // 64) * 64, "head tensors must use row pitch round_up(T, 64) (= packed co_pad)"
    G = B * heads
    conv1d(q.view(1, G * hd, pitch)[:, :, :T], k, G * T, 1, groups=G, out=st.view(1, G * T, st.shape[1])[:, :, :T])
    return st


def softmax_cols(st, G, T, scale):
    check(lib().sat_softmax_columns_f32(ptr(st), G, T, st.shape[1], float(scale), stream()), "sat_softmax_columns_f32")
    return st


def transpose_heads(v, B, heads, hd, T, jpad=None):
    pitch = v.shape[2]
    jpad = jpad or ((T + 15) // 16) * 16
    assert v.is_contiguous()
    vt = torch.empty(B * heads, jpad, hd, dtype=torch.float32, device=v.device)
    check(lib().sat_transpose_heads_f32(ptr(v), ptr(vt), B * heads, hd, T, pitch, jpad, stream()), "sat_transpose_heads_f32")
    return vt


def attention_apply(st, vt, B, heads, hd, T):
    """o[b][h*hd + c][q] = sum_j vt[(b,h)][j][c] * st[(b,h)*T + j][q]: grouped 1x1 conv, packed weights = vt"""
    G = B * heads
    o = torch.empty(B, heads * hd, T, dtype=torch.float32, device=st.device)
    conv1d(st.view(1, G * T, st.shape[1])[:, :, :T], vt, G * hd, 1, groups=G, out=o.view(1, G * hd, T))
    return o


def attention_fused(qs, ks, v, B, heads, hd, T, scale, want_f32=False):
    """fused self-attention on split planes of Q and K and f32 V [B, heads*hd, pitch >= T]: returns (o f32
    [B, heads*hd, T] — unwritten shape carrier unless want_f32 — , o as split planes)"""
    assert v.is_contiguous() and v.shape[1] == heads * hd
    o = torch.empty(B, heads * hd, T, dtype=torch.float32, device=v.device)
    os_ = split_like(B, heads * hd, T, v.device)
    check(lib().sat_attention_f16x3(ptr(qs), ptr(ks), ptr(v), ptr(o) if want_f32 else None, ptr(os_), B, heads, hd, T,
                                    v.shape[2], float(scale), stream()), "sat_attention_f16x3")
    return o, os_


def act_split(x, slope=1.0, out=None, fmt=0):
    """f32 [B][C][T] -> split planes S[b][c/16][hi|lo][(c/8)&1][t][c%8] f16 of lrelu(x, slope)
    (include/satools_hip.h, fmt = SPLIT_F16); fmt = SPLIT_F8 keeps the hi planes and stores e4m3(hi) and
    e4m3(lo * 2^10) bytes in the other two; returned as a [B][C/16][2][2][T][8] float16 tensor (raw 16-byte units)"""
    x = _f32c(x)
    B, c, t = x.shape
    if out is None:
        out = split_like(B, c, t, x.device)
    check(lib().sat_act_split_f32(ptr(x), ptr(out), B, c, t, float(slope), int(fmt), stream()), "sat_act_split_f32")
    return out


def split_like(B, c, t, device):
    return torch.empty(B, c // 16, 2, 2, t, 8, dtype=torch.float16, device=device)


def sidecar_like(B, c, t, device):
    """buffer of the e4m3 sidecar of [B, c, t] split planes: [B][c/16][2 (e4m3(hi) | e4m3(lo * 2^10))][t][16 channels] bytes"""
    return torch.empty(B, c // 16, 2, t, 16, dtype=torch.uint8, device=device)


def planes_f8_sidecar(x_split, out=None):
    """e4m3 sidecar of SPLIT_F16 planes (sat_planes_f8_sidecar): the operand image SAT_CONV_F16F8R reads through x_split8"""
    B, nch, _, _, t, _ = x_split.shape
    if out is None:
        out = sidecar_like(B, nch * 16, t, x_split.device)
    check(lib().sat_planes_f8_sidecar(ptr(x_split), ptr(out), B, nch * 16, t, stream()), "sat_planes_f8_sidecar")
    return out


def conv1d_f8r_supported(x, w_packed, c_out, ksize, **kw):
    d, *_ = _conv1d_desc(x, w_packed, c_out, ksize, **kw)
    return bool(lib().sat_conv1d_f8r_supported(C.byref(d)))


def unsplit(s):
    """split planes -> f32 [B][C][T] (hi + lo); test/debug helper, plain torch"""
    B, nch, _, _, t, _ = s.shape
    v = s[:, :, 0].float() + s[:, :, 1].float()          # [B][nch][half][t][8]
    return v.permute(0, 1, 2, 4, 3).reshape(B, nch * 16, t)


def resblock_pair(x, w1, b1, w2, b2, ksize, dilation, slope=0.1, out=None, accum=False, accum_div=0.0,
                  x_split=None, y_split=None, y_split_slope=1.0, planes_residual=False, no_y=False):
    """fused ResBlock1 step (C = 16 / 32; C = 64 with x_split and planes_residual; split-f16):
    out = conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 + x"""
    x = _f32c(x)
    B, c, t = x.shape
    if out is None:
        out = torch.empty_like(x)
    d = ConvDesc()
    d.B, d.C_in, d.T_in, d.C_out, d.T_q = B, c, t, c, t
    d.ksize, d.dilation, d.stride, d.pad_left, d.groups, d.up, d.mode = ksize, dilation, 1, 0, 1, 1, 1
    d.in_lrelu, d.in_slope = 1, float(slope)
    d.accum, d.accum_div = int(accum), float(accum_div)
    d.res_scale, d.res_toff, d.res_tstride = 1.0, 0, 1
    d.x_bstride, d.x_cstride = x.stride(0), x.stride(1)
    d.y_bstride, d.y_cstride = out.stride(0), out.stride(1)
    d.res_bstride, d.res_cstride = x.stride(0), x.stride(1)
    d.bias, d.res = ptr(b2), (None if planes_residual else ptr(x))
    d.x_split, d.y_split, d.y_split_slope = ptr(x_split), ptr(y_split), float(y_split_slope)
    if planes_residual:
        d.res_split, d.res_split_slope = ptr(x_split), float(slope)
    d.no_y = int(no_y)
    d.w_descale = _descale(w2)
    check(lib().sat_resblock_pair_scaled_f16x3(C.byref(d), None if planes_residual else ptr(x), ptr(w1), ptr(b1),
                                               _descale(w1), ptr(w2), ptr(out), stream()),
          "sat_resblock_pair_scaled_f16x3")
    return out


def resblock_mrf(x_split, B, c, t, branches, slope=0.1, out=None, y_split=None, y_split_slope=1.0, out_div=0.0,
                 residual_from_planes=False):
    """a whole MRF block in one launch (csrc/mrf.hip): `branches` = [(ksize, [(w1, b1, w2, b2) x 3 steps]), ...] with packed
    split-f16 weights; dilations (1, 3, 5); input split planes of lrelu(x, slope); returns the f32 output (or None)"""
    from ._lib import MrfDesc
    d = MrfDesc()
    d.B, d.C, d.T, d.n_branches = B, c, t, len(branches)
    keep = []
    for j, (k, steps) in enumerate(branches):
        d.ksize[j] = k
        for i, (w1, b1, w2, b2) in enumerate(steps):
            d.dilation[j][i] = 2 * i + 1
            d.w[j][i][0], d.w[j][i][1] = ptr(w1), ptr(w2)
            d.bias[j][i][0], d.bias[j][i][1] = ptr(b1), ptr(b2)
            d.w_descale[j][i][0], d.w_descale[j][i][1] = _descale(w1), _descale(w2)
            keep += [w1, b1, w2, b2]
    d.slope = float(slope)
    d.x_split = ptr(x_split)
    if out is None and y_split is None:
        out = torch.empty(B, c, t, dtype=torch.float32, device=x_split.device)
    d.y, d.y_split, d.y_split_slope, d.out_div = ptr(out), ptr(y_split), float(y_split_slope), float(out_div)
    d.residual_from_planes = int(residual_from_planes)
    ks = _lib.int_array([k for k, _ in branches])
    scratch = torch.empty(lib().sat_resblock_mrf_scratch_bytes(len(branches), ks), dtype=torch.uint8, device=x_split.device)
    d.scratch, d.scratch_bytes = ptr(scratch), scratch.numel()
    check(lib().sat_resblock_mrf_f16x3(C.byref(d), stream()), "sat_resblock_mrf_f16x3")
    return out


def upsample2(x_split, w_packed, bias, B, c_in, t, y_split_slope=0.1, y_split=None):
    """ConvTranspose1d(c_in -> c_in / 2, k 4, stride 2, padding 1) on split planes (csrc/ups2.hip): returns the planes of
    lrelu(y, y_split_slope), [B][c_in / 2][2 t]"""
    if y_split is None:
        y_split = split_like(B, c_in // 2, 2 * t, x_split.device)
    check(lib().sat_upsample2_f16x3(ptr(x_split), ptr(w_packed), ptr(bias), _descale(w_packed), ptr(y_split),
                                    float(y_split_slope), B, c_in, t, stream()), "sat_upsample2_f16x3")
    return y_split


# ---- x-vector extractor (csrc/xvector.hip) -------------------------------------------------------
def melspec_logmel(wav, window, fb, coef=0.97):
    """wav [B, n] -> log-mel [B, n_mel, 1 + n // 160]; fb [n_mel, 513] (rows = filters)"""
    wav = _f32c(wav)
    B, n = wav.shape
    n_mel = fb.shape[0]
    lo, hi = mel_filter_ranges(fb)
    out = torch.empty(B, n_mel, 1 + n // 160, dtype=torch.float32, device=wav.device)
    check(lib().sat_melspec_logmel_f32(ptr(wav), ptr(out), ptr(window), ptr(fb), ptr(lo), ptr(hi), B, n,
                                       n_mel, float(coef), stream()), "sat_melspec_logmel_f32")
    return out


def instnorm_rows(x, eps=1e-5):
    x = _f32c(x)
    y = torch.empty_like(x)
    check(lib().sat_instnorm_rows_f32(ptr(x), ptr(y), x.shape[0] * x.shape[1], x.shape[2], float(eps), stream()), "sat_instnorm_rows_f32")
    return y


def row_mean(x):
    """[B, C, T] -> [B, C, 1]: mean over time"""
    x = _f32c(x)
    B, c, t = x.shape
    y = torch.empty(B, c, 1, dtype=torch.float32, device=x.device)
    check(lib().sat_row_mean_f32(ptr(x), ptr(y), B * c, t, stream()), "sat_row_mean_f32")
    return y


def add3(a, b, c=None, out=None):
    """a + b (+ c) on [B, C, T] channel slices (views with T contiguous are fine)"""
    a, b = _strided3(a), _strided3(b)
    c = _strided3(c) if c is not None else None
    B, ch, t = a.shape
    if out is None:
        out = torch.empty(B, ch, t, dtype=torch.float32, device=a.device)
    check(lib().sat_add3_f32(ptr(a, strided=True), ptr(b, strided=True), ptr(c, strided=True), ptr(out, strided=True), B, ch, t,
                             a.stride(0), a.stride(1), b.stride(0), b.stride(1), c.stride(0) if c is not None else 0,
                             c.stride(1) if c is not None else 0, out.stride(0), out.stride(1), stream()), "sat_add3_f32")
    return out


def se_gate_add(z, gate_logits, skips, out=None):
    """z * sigmoid(gate_logits[b, c]) + skips[0] + skips[1] + ...  (up to three skips, added left to right)"""
    z = _f32c(z)
    B, c, t = z.shape
    g = _f32c(gate_logits.reshape(B, c))
    sk = [_f32c(s) for s in skips] + [None] * (3 - len(skips))
    if out is None:
        out = torch.empty_like(z)
    check(lib().sat_se_gate_add_f32(ptr(z), ptr(g), ptr(sk[0]), ptr(sk[1]), ptr(sk[2]), ptr(out, strided=True), B, c, t,
                                    out.stride(0), out.stride(1), stream()), "sat_se_gate_add_f32")
    return out


def tanh_(x):
    check(lib().sat_tanh_inplace_f32(ptr(x), x.numel(), stream()), "sat_tanh_inplace_f32")
    return x


def attentive_stats(x, logits):
    """[B, C, T] x 2 -> [B, 2C, 1]: softmax-weighted mean and std over time"""
    x, logits = _f32c(x), _f32c(logits)
    B, c, t = x.shape
    out = torch.empty(B, 2 * c, 1, dtype=torch.float32, device=x.device)
    check(lib().sat_attentive_stats_f32(ptr(x), ptr(logits), ptr(out), B, c, t, stream()), "sat_attentive_stats_f32")
    return out


def l2norm_rows(x):
    x = _f32c(x)
    y = torch.empty_like(x)
    check(lib().sat_l2norm_rows_f32(ptr(x), ptr(y), x.shape[0], x.shape[1], stream()), "sat_l2norm_rows_f32")
    return y


def res2_chain(y, w, scale, shift, dilation, out=None):
    """Res2Conv1dReluBn on 64-channel pieces in one launch (sidekit/nn.py:74-110): y [B, (nums + 1) * 64, T], w [nums, 3, 64, 64]
    (Conv1d.weight permuted (2, 1, 0) per piece), scale / shift [nums, 64] (the BatchNorm in eval) -> z like y"""
    y = _f32c(y)
    B, C, T = y.shape
    nums = w.shape[0]
    if tuple(w.shape) != (nums, 3, 64, 64) or tuple(scale.shape) != (nums, 64) or tuple(shift.shape) != (nums, 64) or C != (nums + 1) * 64:
        raise _lib.SatError(f"res2_chain: w {tuple(w.shape)} / scale {tuple(scale.shape)} do not fit y {tuple(y.shape)}")
    z = torch.empty_like(y) if out is None else out
    if z.shape != y.shape or not z.is_contiguous() or z.data_ptr() == y.data_ptr():
        raise _lib.SatError("res2_chain: `out` must be a contiguous tensor of y's shape, not y itself")
    check(lib().sat_res2_chain_f32(ptr(y), ptr(z), ptr(_f32c(w)), ptr(_f32c(scale)), ptr(_f32c(shift)), B, C, T, nums, int(dilation), stream()),
          "sat_res2_chain_f32")
    return z


def linear_rows(x, w, bias=None, ch_scale=None, ch_shift=None, relu=False):
    """nn.Linear on pooled vectors: x [B, Cin] (or [B, Cin, 1]), w [Cout, Cin] -> [B, Cout] (or [B, Cout, 1]);
    (relu?)(x w^T + bias) * ch_scale + ch_shift (sidekit/nn.py:133-139, ecapa_tdnn.py:40-43)"""
    col = x.dim() == 3
    if col and x.shape[2] != 1:
        raise _lib.SatError("linear_rows: [B, Cin] or [B, Cin, 1]")
    x2 = _f32c(x.reshape(x.shape[0], x.shape[1]))
    w = _f32c(w)
    B, cin = x2.shape
    cout = w.shape[0]
    if w.dim() != 2 or w.shape[1] != cin or not x2.is_cuda:
        raise _lib.SatError(f"linear_rows: w {tuple(w.shape)} does not fit x {tuple(x2.shape)} on the GPU")
    for t in (bias, ch_scale, ch_shift):
        if t is not None and (t.numel() != cout or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.SatError("linear_rows: bias / ch_scale / ch_shift are contiguous f32 vectors of Cout values")
    y = torch.empty(B, cout, dtype=torch.float32, device=x2.device)
    check(lib().sat_linear_rows_f32(ptr(x2), ptr(w), ptr(bias), ptr(ch_scale), ptr(ch_shift), int(bool(relu)), ptr(y), B, cin, cout, stream()),
          "sat_linear_rows_f32")
    return y.unsqueeze(2) if col else y


# ---- ASR half of the bottleneck net ------------------------------------------------------
def tdnnf_unfold15(x):
    """x [B, D, T] -> (windows, bypass) [B, D, (2(T-1))//3 + 1] of a TDNNF layer with subsampling_factor 1.5"""
    x = _f32c(x)
    B, d, t = x.shape
    tq = (2 * (t - 1)) // 3 + 1
    win = torch.empty(B, d, tq, dtype=torch.float32, device=x.device)
    byp = torch.empty_like(win)
    check(lib().sat_tdnnf_unfold15_f32(ptr(x), ptr(win), ptr(byp), B, d, t, stream()), "sat_tdnnf_unfold15_f32")
    return win, byp


def log_softmax_channels_(x):
    x_ = x
    B, c, t = x_.shape
    check(lib().sat_log_softmax_channels_f32(ptr(x_), B, c, t, stream()), "sat_log_softmax_channels_f32")
    return x_


# ---- ASV evaluation (csrc/asv_score.hip) ---------------------------------------------------------------
def _host_i32(v, what):
    """an index list (anything numpy takes, or a CPU tensor) -> (contiguous int32 numpy array, ctypes pointer)"""
    import numpy as np
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise _lib.SatError(f"{what}: index lists are host arrays (they are checked before the launch)")
        v = v.numpy()
    a = np.asarray(v)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
        raise _lib.SatError(f"{what}: a non-empty one-dimensional integer list is needed, got {a.dtype} {a.shape}")
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise _lib.SatError(f"{what}: values do not fit 32 bits")
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _rows2(t, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda:
        raise _lib.SatError(f"{what}: a two-dimensional float32 device tensor is needed")
    return t.contiguous()


def cohort_topk_stats(x, cohort, k=None):
    """x [N, D], cohort [C, D] -> (mean [N], std [N]) of the k largest of the C dot products of every row (asnorm's topk statistics,
    scoring/__init__.py:25-39; k defaults to min(200, C)); the N x C scores stay in LDS"""
    x, cohort = _rows2(x, "cohort_topk_stats: x"), _rows2(cohort, "cohort_topk_stats: cohort")
    (N, D), (Cn, Dc) = x.shape, cohort.shape
    if D != Dc or N == 0:
        raise _lib.SatError(f"cohort_topk_stats: x {tuple(x.shape)} does not fit cohort {tuple(cohort.shape)}")
    k = min(200, Cn) if k is None else int(k)
    mean = torch.empty(N, dtype=torch.float32, device=x.device)
    std = torch.empty(N, dtype=torch.float32, device=x.device)
    check(lib().sat_cohort_topk_stats_f32(ptr(x), ptr(cohort), N, Cn, D, k, ptr(mean), ptr(std), stream()), "sat_cohort_topk_stats_f32")
    return mean, std


def trial_scores(enroll, test, idx_e, idx_t, stats=None):
    """cosine score of every trial (enroll[idx_e[m]], test[idx_t[m]]) -> score [M]; with stats = (mu_e, sd_e, mu_t, sd_t), the cohort
    statistics of the enrolment and of the test rows, also the adaptive s-norm score [M] -> (score, score_asnorm).
    idx_e / idx_t are host index lists: checked by the entry before anything is launched and copied to the device by a staged
    (pageable) copy, so they may be dropped on return — and the call cannot be recorded into a torch.cuda.graph"""
    enroll, test = _rows2(enroll, "trial_scores: enroll"), _rows2(test, "trial_scores: test")
    ie, pe = _host_i32(idx_e, "trial_scores: idx_e")
    it, pt = _host_i32(idx_t, "trial_scores: idx_t")
    (E, D), (T, Dt) = enroll.shape, test.shape
    if D != Dt or E == 0 or T == 0 or ie.size != it.size:
        raise _lib.SatError(f"trial_scores: enroll {tuple(enroll.shape)}, test {tuple(test.shape)}, {ie.size} and {it.size} indices do not fit")
    M = ie.size
    dev = enroll.device
    st = [None] * 4
    if stats is not None:
        if len(stats) != 4:
            raise _lib.SatError("trial_scores: stats = (mu_e, sd_e, mu_t, sd_t)")
        for i, (s, n) in enumerate(zip(stats, (E, E, T, T))):
            if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or tuple(s.shape) != (n,) or not s.is_cuda:
                raise _lib.SatError(f"trial_scores: statistic {i} must be a float32 device vector of {n} values")
            st[i] = s.contiguous()
    score = torch.empty(M, dtype=torch.float32, device=dev)
    score_as = torch.empty(M, dtype=torch.float32, device=dev) if stats is not None else None
    idx_dev = torch.empty(2 * M, dtype=torch.int32, device=dev)
    check(lib().sat_trial_scores_f32(ptr(enroll), ptr(test), pe, pt, ptr(idx_dev), E, T, M, D, ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]),
                                     ptr(score), ptr(score_as), stream()), "sat_trial_scores_f32")
    return score if stats is None else (score, score_as)


def segment_mean_l2norm(x, order, offsets):
    """x [U, D] -> [S, D]: row s = the mean of x[order[offsets[s]:offsets[s + 1]]] over its L2 norm, or that row itself, bit for bit, when
    the segment holds one (objf.py:272-281).  order / offsets are host index lists (checked and copied like those of trial_scores:
    not for use under torch.cuda.graph)"""
    x = _rows2(x, "segment_mean_l2norm: x")
    o, po = _host_i32(order, "segment_mean_l2norm: order")
    f, pf = _host_i32(offsets, "segment_mean_l2norm: offsets")
    U, D = x.shape
    S = f.size - 1
    if U == 0 or o.size != U or S < 1:
        raise _lib.SatError(f"segment_mean_l2norm: x {tuple(x.shape)}, {o.size} order entries and {f.size} offsets do not fit")
    out = torch.empty(S, D, dtype=torch.float32, device=x.device)
    seg_dev = torch.empty(U + S + 1, dtype=torch.int32, device=x.device)
    check(lib().sat_segment_mean_l2norm_f32(ptr(x), po, pf, ptr(seg_dev), U, S, D, ptr(out), stream()), "sat_segment_mean_l2norm_f32")
    return out


# ---- resampling statistics (csrc/stats/eer_bootstrap.hip, include/satools_hip_stats.h) -----------------
EER_BOOTSTRAP_MAX_SIDE = 1 << 20      # SAT_EER_BOOTSTRAP_MAX_SIDE


def _cut_table(v, n, what):
    """a cut table (host array, CPU or device tensor) -> (int32 numpy copy for the checks, the device tensor it came from or None)"""
    import numpy as np
    dev = None
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            dev = v
        v = v.detach().cpu().numpy()
    a = np.asarray(v)
    if a.ndim != 1 or a.size < 2 or a.dtype.kind not in "iu":
        raise _lib.SatError(f"{what}: a one-dimensional integer table of K + 1 >= 2 values is needed, got {a.dtype} {a.shape}")
    if a.min() < -2 ** 31 or a.max() >= 2 ** 31:
        raise _lib.SatError(f"{what}: values do not fit 32 bits")
    if np.any(np.diff(a.astype(np.int64)) < 0):
        raise _lib.SatError(f"{what}: the counts must not decrease")
    if a[0] < 0 or a[-1] != n:
        raise _lib.SatError(f"{what}: the table must run from a count >= 0 to n = {n}, got {int(a[0])} .. {int(a[-1])}")
    if dev is not None and (dev.dtype != torch.int32 or not dev.is_contiguous()):
        dev = None                    # (uploaded again below, as int32)
    return np.ascontiguousarray(a, dtype=np.int32), dev


def eer_bootstrap(cut_tar, cut_non, n_tar, n_non, m, seed=0, first_replicate=0, device=None):
    """bootstrap replicates first_replicate .. first_replicate + m - 1 of the empirical EER of two score sets given as their cut tables
    (asv_eval.eer_cuts; include/satools_hip_stats.h) -> (miss_at [m], fa_before [m]) int32 device tensors: the replicate's EER is
    min(miss_at / n_tar, fa_before / n_non).  Draws: Philox4x32-10 at the counter (j >> 2, replicate, stream, 0) under the key `seed`,
    word j & 3, mapped to an index by (u n) >> 32 — two indices differ in probability by at most n / 2^32 relative (2.4e-4 at the
    largest n, 2^20).  A replicate depends on (seed, its number) alone.  The tables may be host arrays or device tensors; they are checked
    on the host before the launch (K + 1 values of int32 range, non-decreasing, ending in n, one side starting at 0)."""
    n_tar, n_non, m, seed, first_replicate = int(n_tar), int(n_non), int(m), int(seed), int(first_replicate)
    if n_tar < 1 or n_non < 1 or m < 1:
        raise _lib.SatError(f"eer_bootstrap: n_tar = {n_tar}, n_non = {n_non}, m = {m} must all be at least 1")
    if max(n_tar, n_non) > EER_BOOTSTRAP_MAX_SIDE:
        raise _lib.SatError(f"eer_bootstrap: n_tar = {n_tar}, n_non = {n_non}: a side holds at most {EER_BOOTSTRAP_MAX_SIDE} trials")
    if not 0 <= seed < 2 ** 64:
        raise _lib.SatError(f"eer_bootstrap: seed = {seed} is not a 64-bit unsigned value")
    if first_replicate < 0 or first_replicate + m > 2 ** 31 - 1:
        raise _lib.SatError(f"eer_bootstrap: replicates {first_replicate} .. {first_replicate + m - 1} do not fit 0 .. 2^31 - 1")
    ct, dt = _cut_table(cut_tar, n_tar, "eer_bootstrap: cut_tar")
    cn, dn = _cut_table(cut_non, n_non, "eer_bootstrap: cut_non")
    K = ct.size - 1
    if cn.size != ct.size or K > n_tar + n_non:
        raise _lib.SatError(f"eer_bootstrap: {ct.size} and {cn.size} table entries do not fit K + 1 with K <= n_tar + n_non = {n_tar + n_non}")
    if ct[0] != 0 and cn[0] != 0:
        raise _lib.SatError("eer_bootstrap: no score lies below the smallest threshold: a table must start at 0")
    if device is None:
        device = dt.device if dt is not None else dn.device if dn is not None else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.SatError("eer_bootstrap: the replicates are drawn on the HIP device only (no CPU fallback)")
    dt = dt.to(device) if dt is not None else torch.from_numpy(ct).to(device)
    dn = dn.to(device) if dn is not None else torch.from_numpy(cn).to(device)
    miss_at = torch.empty(m, dtype=torch.int32, device=device)
    fa_before = torch.empty(m, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(lib().sat_eer_bootstrap_i32(ptr(dt), ptr(dn), K, n_tar, n_non, first_replicate, m, seed, ptr(miss_at), ptr(fa_before), stream()),
              "sat_eer_bootstrap_i32")
    return miss_at, fa_before


# ---- ResNet x-vector extractor (csrc/conv2d.hip) -------------------------------------------------------
def pack_conv2d_weight(w, transpose=False):
    """Conv2d.weight [Cout, Cin, k, k] -> the [k * k, Cin, Cout] layout sat_conv2d_f32 reads (tap-major, output channel contiguous).
    `transpose` swaps the two kernel axes: the weight of the same conv on images with their two spatial axes swapped"""
    if w.dim() != 4 or w.shape[2] != w.shape[3] or w.dtype != torch.float32:
        raise _lib.SatError(f"pack_conv2d_weight: a float32 [Cout, Cin, k, k] weight is needed, got {w.dtype} {tuple(w.shape)}")
    if transpose:
        w = w.transpose(2, 3)
    cout, cin, k, _ = w.shape
    return w.permute(2, 3, 1, 0).reshape(k * k, cin, cout).contiguous()


def conv2d(x, w_packed, ksize, stride=1, ch_scale=None, ch_shift=None, relu=False):
    """Conv2d(bias=False, 3x3 with padding 1 or 1x1) + per-channel affine (the BatchNorm in eval) + optional ReLU:
    x [B, Cin, H, W], w_packed from pack_conv2d_weight -> [B, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1]"""
    x = _f32c(x)
    if x.dim() != 4 or w_packed.dim() != 3 or w_packed.dtype != torch.float32 or not w_packed.is_contiguous():
        raise _lib.SatError("conv2d: x [B, Cin, H, W] and packed weights [k * k, Cin, Cout] (pack_conv2d_weight) are needed")
    B, cin, H, W = x.shape
    taps, cin_w, cout = w_packed.shape
    if taps != ksize * ksize or cin_w != cin:
        raise _lib.SatError(f"conv2d: packed weights {tuple(w_packed.shape)} do not fit x {tuple(x.shape)} with ksize {ksize}")
    for t in (ch_scale, ch_shift):
        if t is not None and (t.numel() != cout or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.SatError("conv2d: ch_scale / ch_shift are contiguous f32 vectors of Cout values")
    stride = int(stride)
    if stride < 1:
        raise _lib.SatError("conv2d: stride 1 or 2")
    y = torch.empty(B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1, dtype=torch.float32, device=x.device)
    check(lib().sat_conv2d_f32(ptr(x), ptr(w_packed), ptr(y), ptr(ch_scale), ptr(ch_shift), int(bool(relu)), B, cin, cout, H, W, int(ksize),
                               stride, stream()), "sat_conv2d_f32")
    return y


def pack_conv2d_weight_f16x3(w, transpose=False):
    """Conv2d.weight [Cout, Cin, k, k] float32 -> (w_split, descale) for sat_conv2d_f16x3_f32 (include/satools_hip_conv2d16.h):
    w_split = f16 [Cin / 16, k * k, 2 (hi | lo), 2 (channel half), Cout, 8] of w' = w * 2^e — hi = f16(w'), lo = f16(w' - hi) — with the
    per-layer scale of packing.pack_conv_weight_f16x3 (the largest |w'| in [2^9, 2^10); e = 0 for an all-zero weight), descale = 2^-e.
    `transpose` swaps the two kernel axes, as in pack_conv2d_weight.  Non-finite weights raise packing.SplitRangeError"""
    from . import packing
    if w.dim() != 4 or w.shape[2] != w.shape[3] or w.dtype != torch.float32:
        raise _lib.SatError(f"pack_conv2d_weight_f16x3: a float32 [Cout, Cin, k, k] weight is needed, got {w.dtype} {tuple(w.shape)}")
    if w.shape[1] % 16 != 0:
        raise _lib.SatError(f"pack_conv2d_weight_f16x3: Cin = {w.shape[1]} is not a multiple of 16")
    if transpose:
        w = w.transpose(2, 3)
    e = packing.f16x3_scale_exponent(w)
    cout, cin, k, _ = w.shape
    p = w.detach() * float(2.0 ** e)                                              # (a power of two: exact)
    p = p.reshape(cout, cin // 16, 2, 8, k * k).permute(1, 4, 2, 0, 3).contiguous()      # [chunk][tap][half][co][8]
    hi = p.to(torch.float16)
    lo = (p - hi.to(torch.float32)).to(torch.float16)
    return torch.stack([hi, lo], dim=2).contiguous(), float(2.0 ** -e)


def conv2d_f16x3(x, w_split, descale, ksize, stride=1, ch_scale=None, ch_shift=None, relu=False, overflow=None):
    """conv2d in split-f16 arithmetic (three f16 MFMA products per term, f32 accumulation): x [B, Cin, H, W] f32, (w_split, descale) from
    pack_conv2d_weight_f16x3 -> [B, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1] f32.  `overflow`: an int32 tensor of one element
    on x's device, or None; the kernel makes it nonzero if a staged activation had |x| >= 65 520 or was not finite (the results are then
    unspecified), and never clears it"""
    x = _f32c(x)
    if x.dim() != 4 or w_split.dim() != 6 or w_split.dtype != torch.float16 or not w_split.is_contiguous():
        raise _lib.SatError("conv2d_f16x3: x [B, Cin, H, W] and split weights f16 [Cin / 16, k * k, 2, 2, Cout, 8] (pack_conv2d_weight_f16x3) are needed")
    B, cin, H, W = x.shape
    chunks, taps, parts, halves, cout, eight = w_split.shape
    if taps != ksize * ksize or chunks * 16 != cin or (parts, halves, eight) != (2, 2, 8):
        raise _lib.SatError(f"conv2d_f16x3: split weights {tuple(w_split.shape)} do not fit x {tuple(x.shape)} with ksize {ksize}")
    for t in (ch_scale, ch_shift):
        if t is not None and (t.numel() != cout or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.SatError("conv2d_f16x3: ch_scale / ch_shift are contiguous f32 vectors of Cout values")
    stride = int(stride)
    if stride < 1:
        raise _lib.SatError("conv2d_f16x3: stride 1 or 2")
    descale = float(descale)
    if not (0.0 < descale < float("inf")):
        raise _lib.SatError(f"conv2d_f16x3: descale = {descale} (the 2^-e pack_conv2d_weight_f16x3 returned)")
    if overflow is not None and (overflow.dtype != torch.int32 or overflow.numel() != 1 or overflow.device != x.device):
        raise _lib.SatError("conv2d_f16x3: overflow is one int32 on x's device")
    y = torch.empty(B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1, dtype=torch.float32, device=x.device)
    check(lib().sat_conv2d_f16x3_f32(ptr(x), ptr(w_split), descale, ptr(y), ptr(ch_scale), ptr(ch_shift), int(bool(relu)), B, cin, cout, H, W,
                                     int(ksize), stride, ptr(overflow), stream()), "sat_conv2d_f16x3_f32")
    return y


def se_scale_add_relu(z, gate_logits, r):
    """relu(z * sigmoid(gate_logits[b, c]) + r): the tail of ResNetBasicBlock.forward; z, r [B, C, ...] of one shape"""
    z, r = _f32c(z), _f32c(r)
    if z.dim() < 3 or z.shape != r.shape:
        raise _lib.SatError(f"se_scale_add_relu: z {tuple(z.shape)} and r {tuple(r.shape)} must be [B, C, ...] of one shape")
    B, c = z.shape[:2]
    g = _f32c(gate_logits.reshape(B, c))
    y = torch.empty_like(z)
    check(lib().sat_se_scale_add_relu_f32(ptr(z), ptr(g), ptr(r), ptr(y), B, c, z.numel() // (B * c), stream()), "sat_se_scale_add_relu_f32")
    return y


def row_mean_std(x):
    """[B, C, T] -> [B, 2C]: mean and unbiased standard deviation over time (MeanStdPooling), means first"""
    x = _f32c(x)
    if x.dim() != 3:
        raise _lib.SatError("row_mean_std: [B, C, T]")
    B, c, t = x.shape
    out = torch.empty(B, 2 * c, dtype=torch.float32, device=x.device)
    check(lib().sat_row_mean_std_f32(ptr(x), ptr(out), B, c, t, stream()), "sat_row_mean_std_f32")
    return out


# ---- ragged batches of the x-vector extractor (csrc/ragged/, include/satools_hip_ragged.h) ---------------------------------------
RAGGED_GAP, RAGGED_ALIGN, RAGGED_MAX_SEGMENTS = 2, 4, 1024
XV_HOP, XV_MIN_SAMPLES = 160, 513             # csrc/xvector.hip: frames = 1 + n // 160; the reflect padding needs n > 512


def ragged_layout(frames):
    """the packed time axis of a ragged batch (include/satools_hip_ragged.h): frames [B] -> (seg_off [B], seg_len [B], T_tot), int32 numpy.
    off_0 = 0, off_{i+1} = round_up(off_i + T_i + 2, 4), T_tot = off_B: at least 2 gap columns after every segment, the last included,
    every segment on a multiple of 4 columns.  Pure host code."""
    import numpy as np
    frames = [int(t) for t in frames]
    if not frames or len(frames) > RAGGED_MAX_SEGMENTS or min(frames) < 1:
        raise _lib.SatError(f"ragged_layout: 1 .. {RAGGED_MAX_SEGMENTS} segments of at least one frame each, got {len(frames)}"
                            + (f" with a segment of {min(frames)}" if frames else ""))
    off, pos = [], 0
    for t in frames:
        off.append(pos)
        pos = -(-(pos + t + RAGGED_GAP) // RAGGED_ALIGN) * RAGGED_ALIGN
    if pos >= 2 ** 31:
        raise _lib.SatError("ragged_layout: 2^31 columns or more")
    return np.asarray(off, dtype=np.int32), np.asarray(frames, dtype=np.int32), pos


def ragged_tiles(frames):
    """the tile table of sat_res2_chain_segments_f32: int32 pairs (segment, first column inside it) for 64-column centres, then for
    128-column centres -> (tiles [n64 + n128, 2], n64, n128)"""
    import numpy as np
    pairs = [(i, t0) for centre in (64, 128) for i, t in enumerate(frames) for t0 in range(0, int(t), centre)]
    n64 = sum(-(-int(t) // 64) for t in frames)
    return np.asarray(pairs, dtype=np.int32).reshape(-1, 2), n64, len(pairs) - n64


class _PinnedRing:
    """page-locked int32 blocks for the tables of ragged batches, reused in turn (f0._PinnedInts explains why not `pin_memory()` per call).
    A block is written again SLOTS uploads later, after the event behind its last copy: a host that runs that far ahead waits for a copy
    issued four batches ago, never for a kernel."""
    SLOTS = 4

    def __init__(self):
        import threading
        self.slots, self.next, self.lock = [None] * self.SLOTS, 0, threading.Lock()

    def upload(self, words, device):
        """int32 numpy vector -> device tensor, one asynchronous copy on the current stream"""
        n = int(words.size)
        with self.lock:
            k, self.next = self.next, (self.next + 1) % self.SLOTS
            slot = self.slots[k]
            if slot is not None:
                slot[1].synchronize()
            if slot is None or slot[0].numel() < n:
                slot = [torch.empty(max(n, 8192), dtype=torch.int32, pin_memory=True), None]
            slot[0][:n].copy_(torch.from_numpy(words))
            dev = torch.empty(n, dtype=torch.int32, device=device)
            dev.copy_(slot[0][:n], non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record(torch.cuda.current_stream(device))
            self.slots[k] = slot
        return dev


_ragged_ring = _PinnedRing()


class RaggedTable:
    """the tables of one ragged batch: built on the host from the known lengths, on the device after ONE copy.
    `n_samples` [B] (frames = 1 + n // 160) or `frames` [B] alone (for the kernels past the front end)"""

    def __init__(self, device, n_samples=None, frames=None):
        import numpy as np
        if n_samples is not None:
            n_samples = [int(n) for n in n_samples]
            frames = [1 + max(n, 0) // XV_HOP for n in n_samples]
        else:
            frames = [int(t) for t in frames]
            n_samples = [(t - 1) * XV_HOP for t in frames]
        off, length, self.T_tot = ragged_layout(frames)
        tiles, self.n_tiles64, self.n_tiles128 = ragged_tiles(frames)
        self.B, self.frames, self.n_samples_list = len(frames), frames, n_samples
        self.host_off, self.host_len = off, length
        self.n_samples_host = (C.c_int32 * self.B)(*n_samples)
        B = self.B
        dev = _ragged_ring.upload(np.concatenate([off, length, np.asarray(n_samples, dtype=np.int32), tiles.reshape(-1)]), device)
        self.seg_off, self.seg_len, self.n_samples, self.tiles = dev[:B], dev[B:2 * B], dev[2 * B:3 * B], dev[3 * B:]

    def segment(self, x, i):
        """the columns of segment i of a packed tensor [..., T_tot]"""
        return x[..., int(self.host_off[i]):int(self.host_off[i]) + int(self.host_len[i])]


def _packed2(t, tab, what):
    """[1, C, T_tot] or [C, T_tot] f32 on the device -> (C, the tensor made contiguous)"""
    t = _f32c(t)
    if t.dim() == 3 and t.shape[0] == 1:
        c = t.shape[1]
    elif t.dim() == 2:
        c = t.shape[0]
    else:
        raise _lib.SatError(f"{what}: a packed tensor is [1, C, T_tot] or [C, T_tot], got {tuple(t.shape)}")
    if t.shape[-1] != tab.T_tot:
        raise _lib.SatError(f"{what}: {t.shape[-1]} columns, the table has T_tot = {tab.T_tot}")
    return c, t


def mel_filter_ranges(fb):
    """first and one-past-last nonzero bin of every filter of fb [n_mel, 513] -> (lo, hi) int32 on fb's device: the bins the kernels' mel dot
    products run over"""
    n_mel = fb.shape[0]
    nz = fb > 0
    lo = torch.where(nz.any(1), nz.float().argmax(1), torch.zeros(n_mel, dtype=torch.long, device=fb.device)).to(torch.int32)
    hi = torch.where(nz.any(1), fb.shape[1] - torch.flip(nz, [1]).float().argmax(1),
                     torch.zeros(n_mel, dtype=torch.long, device=fb.device)).to(torch.int32)
    return lo.contiguous(), hi.contiguous()


def melspec_logmel_segments(wav, tab, window, fb, coef=0.97, fb_range=None):
    """wav [B, n_max] (anything past n_i) -> log-mel [1, n_mel, T_tot], utterance i at its own length in segment i; gap columns unwritten"""
    wav = _f32c(wav)
    if wav.dim() != 2 or wav.shape[0] != tab.B:
        raise _lib.SatError(f"melspec_logmel_segments: wav {tuple(wav.shape)} against a table of {tab.B} utterances")
    B, n_max = wav.shape
    n_mel = fb.shape[0]
    lo, hi = fb_range if fb_range is not None else mel_filter_ranges(fb)
    out = torch.empty(1, n_mel, tab.T_tot, dtype=torch.float32, device=wav.device)
    check(lib().sat_melspec_logmel_segments_f32(ptr(wav), ptr(tab.n_samples), tab.n_samples_host, ptr(tab.seg_off), ptr(tab.seg_len), ptr(out),
                                                ptr(window), ptr(fb), ptr(lo), ptr(hi), B, n_max, tab.T_tot, n_mel, float(coef), stream()),
          "sat_melspec_logmel_segments_f32")
    return out


def instnorm_segments(x, tab, eps=1e-5, out=None):
    """InstanceNorm per (row, segment) of a packed tensor; the gap columns of the result are zeros"""
    c, x = _packed2(x, tab, "instnorm_segments")
    y = torch.empty_like(x) if out is None else out
    check(lib().sat_instnorm_segments_f32(ptr(x), ptr(y), ptr(tab.seg_off), ptr(tab.seg_len), c, tab.B, tab.T_tot, float(eps), stream()),
          "sat_instnorm_segments_f32")
    return y


def row_mean_segments(x, tab):
    """packed [1, C, T_tot] -> [B, C]: mean over each segment"""
    c, x = _packed2(x, tab, "row_mean_segments")
    y = torch.empty(tab.B, c, dtype=torch.float32, device=x.device)
    check(lib().sat_row_mean_segments_f32(ptr(x), ptr(y), ptr(tab.seg_off), ptr(tab.seg_len), c, tab.B, tab.T_tot, stream()),
          "sat_row_mean_segments_f32")
    return y


def se_gate_add_segments(z, gate_logits, skips, tab, out=None):
    """z * sigmoid(gate_logits[i, c]) + skips[0] + skips[1] + ... on the columns of segment i (up to three skips, left to right); `out` may be a
    channel slice of a wider packed tensor; its gap columns are not written"""
    c, z = _packed2(z, tab, "se_gate_add_segments")
    g = _f32c(gate_logits.reshape(tab.B, c))
    sk = [_packed2(s, tab, "se_gate_add_segments")[1] for s in skips] + [None] * (3 - len(skips))
    if out is None:
        out = torch.empty_like(z)
    if out.shape[-2:] != z.shape[-2:] or out.stride(-1) != 1 or out.numel() != z.numel():
        raise _lib.SatError(f"se_gate_add_segments: out {tuple(out.shape)} for z {tuple(z.shape)}")
    check(lib().sat_se_gate_add_segments_f32(ptr(z), ptr(g), ptr(sk[0]), ptr(sk[1]), ptr(sk[2]), ptr(out, strided=True), ptr(tab.seg_off),
                                             ptr(tab.seg_len), c, tab.B, tab.T_tot, out.stride(-2), stream()), "sat_se_gate_add_segments_f32")
    return out


def attentive_stats_segments(x, logits, tab):
    """packed x, logits [1, C, T_tot] -> [B, 2C]: softmax-weighted mean and std over each segment"""
    c, x = _packed2(x, tab, "attentive_stats_segments")
    c2, logits = _packed2(logits, tab, "attentive_stats_segments")
    if c2 != c:
        raise _lib.SatError("attentive_stats_segments: x and logits of different channel counts")
    out = torch.empty(tab.B, 2 * c, dtype=torch.float32, device=x.device)
    check(lib().sat_attentive_stats_segments_f32(ptr(x), ptr(logits), ptr(out), ptr(tab.seg_off), ptr(tab.seg_len), c, tab.B, tab.T_tot, stream()),
          "sat_attentive_stats_segments_f32")
    return out


def res2_chain_segments(y, w, scale, shift, dilation, tab, centre=0, out=None):
    """ops.res2_chain with every segment of the packed y [1, (nums + 1) * 64, T_tot] an utterance of its own; centre = 0 (automatic), 64 or
    128 columns per block.  Gap columns of the result are not written."""
    C_, y = _packed2(y, tab, "res2_chain_segments")
    nums = w.shape[0]
    if tuple(w.shape) != (nums, 3, 64, 64) or tuple(scale.shape) != (nums, 64) or tuple(shift.shape) != (nums, 64) or C_ != (nums + 1) * 64:
        raise _lib.SatError(f"res2_chain_segments: w {tuple(w.shape)} / scale {tuple(scale.shape)} do not fit y {tuple(y.shape)}")
    z = torch.empty_like(y) if out is None else out
    if z.shape != y.shape or not z.is_contiguous() or z.data_ptr() == y.data_ptr():
        raise _lib.SatError("res2_chain_segments: `out` must be a contiguous tensor of y's shape, not y itself")
    check(lib().sat_res2_chain_segments_f32(ptr(y), ptr(z), ptr(_f32c(w)), ptr(_f32c(scale)), ptr(_f32c(shift)), ptr(tab.seg_off), ptr(tab.seg_len),
                                            ptr(tab.tiles), tab.n_tiles64, tab.n_tiles128, tab.B, C_, tab.T_tot, nums, int(dilation), int(centre),
                                            stream()), "sat_res2_chain_segments_f32")
    return z


# ---- ragged batches of the ResNet x-vector extractor (csrc/ragged2d/, include/satools_hip_ragged2d.h) ------------------------------
RESNET_LEVELS = 4                             # time resolutions of the half-ResNet34: the stem and layer1, then one per stride-2 layer


def ragged_levels(frames):
    """the packed time axes of a ragged batch at the ResNet's four time resolutions (include/satools_hip_ragged2d.h): frames [B] ->
    [(seg_off [B], seg_len [B], T_tot)] * 4, level l + 1 holding (T - 1) // 2 + 1 frames of every T of level l, each level laid out by
    ragged_layout on its own.  Pure host code."""
    levels, frames = [], [int(t) for t in frames]
    for _ in range(RESNET_LEVELS):
        levels.append(ragged_layout(frames))
        frames = [(t - 1) // 2 + 1 for t in frames]
    return levels


def ragged_column_segments(off, length, t_tot):
    """column -> segment of one packed axis, int32 [T_tot]: i on the columns of segment i; a gap column names the segment before it
    (any valid row would do: nothing reads what is gathered there)"""
    import numpy as np
    return (np.searchsorted(np.asarray(off), np.arange(int(t_tot)), side="right") - 1).astype(np.int32)


class RaggedLevel:
    """one packed time axis: what the segment kernels need of a RaggedTable.  `off`, `length` int32 numpy [B] and T_tot; the device
    copies are given (RaggedLevels: slices of its one upload) or made here (a table of one's own, a blocking copy)"""

    def __init__(self, off, length, t_tot, seg_off=None, seg_len=None, device=None):
        import numpy as np
        off, length = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(length, dtype=np.int32)
        if seg_off is None:
            seg_off, seg_len = torch.from_numpy(off.copy()).to(device), torch.from_numpy(length.copy()).to(device)
        self.host_off, self.host_len, self.T_tot, self.seg_off, self.seg_len = off, length, int(t_tot), seg_off, seg_len
        self.B, self.frames = len(off), [int(n) for n in length]

    segment = RaggedTable.segment


class RaggedLevels:
    """the tables of one ragged batch of the ResNet extractor, one per time resolution: built on the host from the known lengths, on the
    device after ONE asynchronous copy (the ring of RaggedTable); nothing waits for the device.  `n_samples` [B] (frames = 1 + n // 160)
    or `frames` [B] alone.  levels[0] serves wherever a RaggedTable does in the front end (melspec_logmel_segments, instnorm_segments);
    `columns` is the column -> segment index of the last level (int32 [T_tot_3])."""

    def __init__(self, device, n_samples=None, frames=None):
        import numpy as np
        if n_samples is not None:
            n_samples = [int(n) for n in n_samples]
            frames = [1 + max(n, 0) // XV_HOP for n in n_samples]
        else:
            frames = [int(t) for t in frames]
            n_samples = [(t - 1) * XV_HOP for t in frames]
        host = ragged_levels(frames)
        B = self.B = len(frames)
        col = ragged_column_segments(*host[-1])
        dev = _ragged_ring.upload(np.concatenate([a for off, length, _ in host for a in (off, length)]
                                                 + [np.asarray(n_samples, dtype=np.int32), col]), device)
        self.levels = [RaggedLevel(off, length, t, dev[2 * l * B:(2 * l + 1) * B], dev[(2 * l + 1) * B:(2 * l + 2) * B])
                       for l, (off, length, t) in enumerate(host)]
        first = self.levels[0]
        first.n_samples, first.n_samples_list, first.n_samples_host = dev[8 * B:9 * B], n_samples, (C.c_int32 * B)(*n_samples)
        self.columns = dev[9 * B:]

    def __getitem__(self, l):
        return self.levels[l]


def _packed3(t, tab, what):
    """[1, C, H, T_tot] or [C, H, T_tot] f32 on the device -> (C, H, the tensor made contiguous)"""
    t = _f32c(t)
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3:
        raise _lib.SatError(f"{what}: a packed image is [1, C, H, T_tot] or [C, H, T_tot], got {tuple(t.shape)}")
    if t.shape[-1] != tab.T_tot:
        raise _lib.SatError(f"{what}: {t.shape[-1]} columns, the table has T_tot = {tab.T_tot}")
    return t.shape[0], t.shape[1], t


def conv2d_segments(x, w_packed, ksize, stride, tab_in, tab_out, ch_scale=None, ch_shift=None, relu=False, out=None):
    """ops.conv2d with every segment of the packed image x [1, Cin, H, T_in] an utterance of its own -> [1, Cout, Ho, T_out]: segment i
    of `tab_in` (W_i columns) goes to segment i of `tab_out`, which holds (W_i - 1) // stride + 1 columns (the same table at stride 1, the
    next level's at stride 2; any table of those lengths does).  Gap columns of the result are not written."""
    cin, H, x = _packed3(x, tab_in, "conv2d_segments")
    if w_packed.dim() != 3 or w_packed.dtype != torch.float32 or not w_packed.is_contiguous():
        raise _lib.SatError("conv2d_segments: packed weights [k * k, Cin, Cout] (pack_conv2d_weight) are needed")
    taps, cin_w, cout = w_packed.shape
    stride = int(stride)
    if taps != ksize * ksize or cin_w != cin or stride < 1:
        raise _lib.SatError(f"conv2d_segments: packed weights {tuple(w_packed.shape)} do not fit x {tuple(x.shape)} with ksize {ksize}, stride {stride}")
    for t in (ch_scale, ch_shift):
        if t is not None and (t.numel() != cout or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.SatError("conv2d_segments: ch_scale / ch_shift are contiguous f32 vectors of Cout values")
    if tab_out.B != tab_in.B or [(n - 1) // stride + 1 for n in tab_in.frames] != tab_out.frames:
        raise _lib.SatError(f"conv2d_segments: the output table's segments are not the input's at stride {stride}")
    Ho = (H - 1) // stride + 1
    y = torch.empty(1, cout, Ho, tab_out.T_tot, dtype=torch.float32, device=x.device) if out is None else out
    if tuple(y.shape[-3:]) != (cout, Ho, tab_out.T_tot) or y.numel() != cout * Ho * tab_out.T_tot or y.dtype != torch.float32:
        raise _lib.SatError(f"conv2d_segments: out {tuple(y.shape)} is not [1, {cout}, {Ho}, {tab_out.T_tot}]")
    check(lib().sat_conv2d_segments_f32(ptr(x), ptr(w_packed), ptr(y), ptr(ch_scale), ptr(ch_shift), int(bool(relu)), ptr(tab_in.seg_off),
                                        ptr(tab_in.seg_len), ptr(tab_out.seg_off), tab_in.B, max(tab_in.frames), cin, cout, H, tab_in.T_tot,
                                        tab_out.T_tot, int(ksize), stride, stream()), "sat_conv2d_segments_f32")
    return y


def plane_mean_segments(x, tab):
    """packed [1, C, H, T_tot] -> [B, C]: the mean over the H x T_i plane of each segment (the SE squeeze)"""
    c, H, x = _packed3(x, tab, "plane_mean_segments")
    y = torch.empty(tab.B, c, dtype=torch.float32, device=x.device)
    check(lib().sat_plane_mean_segments_f32(ptr(x), ptr(y), ptr(tab.seg_off), ptr(tab.seg_len), c, H, tab.B, tab.T_tot, stream()),
          "sat_plane_mean_segments_f32")
    return y


def se_scale_add_relu_segments(z, gate_logits, r, tab, out=None):
    """relu(z * sigmoid(gate_logits[i, c]) + r) on the columns of segment i; z, r packed [1, C, H, T_tot]; gap columns of the result are
    not written"""
    c, H, z = _packed3(z, tab, "se_scale_add_relu_segments")
    c2, H2, r = _packed3(r, tab, "se_scale_add_relu_segments")
    if (c2, H2) != (c, H):
        raise _lib.SatError(f"se_scale_add_relu_segments: z {tuple(z.shape)} and r {tuple(r.shape)} must be of one shape")
    g = _f32c(gate_logits.reshape(tab.B, c))
    y = torch.empty(1, c, H, tab.T_tot, dtype=torch.float32, device=z.device) if out is None else out
    if y.numel() != z.numel() or y.dtype != torch.float32:
        raise _lib.SatError(f"se_scale_add_relu_segments: out {tuple(y.shape)} for z {tuple(z.shape)}")
    check(lib().sat_se_scale_add_relu_segments_f32(ptr(z), ptr(g), ptr(r), ptr(y), ptr(tab.seg_off), ptr(tab.seg_len), tab.B, max(tab.frames), c, H,
                                                   tab.T_tot, stream()), "sat_se_scale_add_relu_segments_f32")
    return y


def row_mean_std_segments(x, tab):
    """packed [1, R, T_tot] -> [B, 2R]: mean and unbiased standard deviation over each segment, means first.  A segment of one column has
    no unbiased deviation and is refused"""
    c, x = _packed2(x, tab, "row_mean_std_segments")
    if min(tab.frames) < 2:
        raise _lib.SatError(f"row_mean_std_segments: segment {tab.frames.index(min(tab.frames))} of {min(tab.frames)} column: the unbiased deviation needs two")
    out = torch.empty(tab.B, 2 * c, dtype=torch.float32, device=x.device)
    check(lib().sat_row_mean_std_segments_f32(ptr(x), ptr(out), ptr(tab.seg_off), ptr(tab.seg_len), c, tab.B, tab.T_tot, stream()),
          "sat_row_mean_std_segments_f32")
    return out


# ---- split-f16 2-D convs in ragged batches (csrc/ragged2d16/, include/satools_hip_ragged2d16.h) ------------------------------------
def conv2d_f16x3_segments(x, w_split, descale, ksize, stride, tab_in, tab_out, ch_scale=None, ch_shift=None, relu=False, overflow=None, out=None):
    """ops.conv2d_f16x3 with every segment of the packed image x [1, Cin, H, T_in] an utterance of its own -> [1, Cout, Ho, T_out], the
    tables as for ops.conv2d_segments: segment i of the result has the bits of ops.conv2d_f16x3 on utterance i alone.  (w_split, descale)
    from pack_conv2d_weight_f16x3.  `overflow`: an int32 tensor of tab_in.B elements on x's device, or None; the kernel makes element i
    nonzero if a staged activation of segment i had |x| >= 65 520 or was not finite (that segment's results are then unspecified), and
    never clears one.  Gap columns of x raise no flag and reach no result; gap columns of the result are not written."""
    cin, H, x = _packed3(x, tab_in, "conv2d_f16x3_segments")
    if w_split.dim() != 6 or w_split.dtype != torch.float16 or not w_split.is_contiguous():
        raise _lib.SatError("conv2d_f16x3_segments: split weights f16 [Cin / 16, k * k, 2, 2, Cout, 8] (pack_conv2d_weight_f16x3) are needed")
    chunks, taps, parts, halves, cout, eight = w_split.shape
    stride = int(stride)
    if taps != ksize * ksize or chunks * 16 != cin or (parts, halves, eight) != (2, 2, 8) or stride < 1:
        raise _lib.SatError(f"conv2d_f16x3_segments: split weights {tuple(w_split.shape)} do not fit x {tuple(x.shape)} with ksize {ksize}, stride {stride}")
    for t in (ch_scale, ch_shift):
        if t is not None and (t.numel() != cout or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.SatError("conv2d_f16x3_segments: ch_scale / ch_shift are contiguous f32 vectors of Cout values")
    descale = float(descale)
    if not (0.0 < descale < float("inf")):
        raise _lib.SatError(f"conv2d_f16x3_segments: descale = {descale} (the 2^-e pack_conv2d_weight_f16x3 returned)")
    if tab_out.B != tab_in.B or [(n - 1) // stride + 1 for n in tab_in.frames] != tab_out.frames:
        raise _lib.SatError(f"conv2d_f16x3_segments: the output table's segments are not the input's at stride {stride}")
    if overflow is not None and (overflow.dtype != torch.int32 or overflow.numel() != tab_in.B or overflow.device != x.device or not overflow.is_contiguous()):
        raise _lib.SatError(f"conv2d_f16x3_segments: overflow is {tab_in.B} contiguous int32 (one per segment) on x's device")
    Ho = (H - 1) // stride + 1
    y = torch.empty(1, cout, Ho, tab_out.T_tot, dtype=torch.float32, device=x.device) if out is None else out
    if tuple(y.shape[-3:]) != (cout, Ho, tab_out.T_tot) or y.numel() != cout * Ho * tab_out.T_tot or y.dtype != torch.float32:
        raise _lib.SatError(f"conv2d_f16x3_segments: out {tuple(y.shape)} is not [1, {cout}, {Ho}, {tab_out.T_tot}]")
    check(lib().sat_conv2d_f16x3_segments_f32(ptr(x), ptr(w_split), descale, ptr(y), ptr(ch_scale), ptr(ch_shift), int(bool(relu)), ptr(tab_in.seg_off),
                                              ptr(tab_in.seg_len), ptr(tab_out.seg_off), tab_in.B, max(tab_in.frames), cin, cout, H, tab_in.T_tot,
                                              tab_out.T_tot, int(ksize), stride, ptr(overflow), stream()), "sat_conv2d_f16x3_segments_f32")
    return y
