"""wav2vec2-large front end + TDNNF tail + VQ bottleneck behind the reference's
`tdnnf_wav2vec2_vq.Net.extract_bn` (egs/asr/librispeech/local/chain/tuning/tdnnf_wav2vec2_vq.py:21-345).

The wav2vec2 model itself is torchaudio's (`import_fairseq_model.py:81-113`), third-party to the
reference and absent here: its module semantics are restated from torchaudio 2.1 (oracle/wav2vec2.py) and
cross-checked layer by layer against HF transformers' stable-layer-norm Wav2Vec2Model, the architecture
torchaudio's own importer maps one-to-one onto this configuration (tests/golden/fx_w2v2_hf.npz).  Parameters keep torchaudio's state-dict key names
(`preprocessor.feature_extractor...`, `preprocessor.encoder...`) so reference checkpoints load.

Everything runs on the HIP kernels with activations channel-major [B][C][T]:
  * conv layer 0 (1 -> 512, k 10, stride 5): dedicated streaming kernel;
  * the six stride-2 convs: the LayerNorm+GELU kernel writes its output split into even/odd time phases
    (2C channels, T/2 frames), which turns a stride-2 conv of k taps into a stride-1 conv of ceil(k/2) taps
    on the fused MFMA conv kernel;
  * every Linear = 1x1 conv (bias / GELU / residual in the epilogue), in split-f16 through the GEMM kernel, its
    input handed over as split planes by the LayerNorm / attention / previous Linear that produced it;
  * attention, split-f16: one fused kernel per layer (Q, K as split planes from their projections, scores and
    softmax in registers — a running softmax over blocks of 256 keys —, context out as split planes); f32 mode: S^T = K^T Q and O = V P as GROUPED convs, one
    group per (utterance, head) — a [64][T] head slice of Q / of V^T stored with row pitch 256 is exactly the
    exact-f32 kernel's packed-weight layout — with a column softmax kernel in between.
"""
import os

import torch
import torch.nn as nn

from . import _lib, ops, packing
from .asrbn import _AsrHead, _TdnnfBase, get_padding
from .params import WeightNormConv, _p, tdnnf_stack

CONV_LAYERS = [(512, 10, 5), (512, 3, 2), (512, 3, 2), (512, 3, 2), (512, 3, 2), (512, 2, 2), (512, 2, 2)]


class _WB(nn.Module):
    def __init__(self, *wshape, bias=None):
        super().__init__()
        self.weight = _p(*wshape)
        self.bias = _p(bias if bias is not None else wshape[0])


class _ConvBlock(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = _WB(cout, cin, k)
        self.layer_norm = _WB(cout)


class _FeatureExtractor(nn.Module):
    def __init__(self):
        super().__init__()
        blocks, cin = [], 1
        for cout, k, _ in CONV_LAYERS:
            blocks.append(_ConvBlock(cin, cout, k))
            cin = cout
        self.conv_layers = nn.ModuleList(blocks)


class _FeatureProjection(nn.Module):
    def __init__(self):
        super().__init__()
        self.layer_norm = _WB(512)
        self.projection = _WB(1024, 512)


class _PosConvHolder(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Module()
        self.conv.bias = _p(1024)
        self.conv.weight_g = _p(1, 1, 128)
        self.conv.weight_v = _p(1024, 64, 128)


class _Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self.k_proj = _WB(1024, 1024)
        self.v_proj = _WB(1024, 1024)
        self.q_proj = _WB(1024, 1024)
        self.out_proj = _WB(1024, 1024)


class _FeedForward(nn.Module):
    def __init__(self):
        super().__init__()
        self.intermediate_dense = _WB(4096, 1024)
        self.output_dense = _WB(1024, 4096)


class _EncoderLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.attention = _Attention()
        self.layer_norm = _WB(1024)
        self.feed_forward = _FeedForward()
        self.final_layer_norm = _WB(1024)


class _Transformer(nn.Module):
    def __init__(self, n_layers):
        super().__init__()
        self.pos_conv_embed = _PosConvHolder()
        self.layer_norm = _WB(1024)
        self.layers = nn.ModuleList([_EncoderLayer() for _ in range(n_layers)])


class _Encoder(nn.Module):
    def __init__(self, n_layers):
        super().__init__()
        self.feature_projection = _FeatureProjection()
        self.transformer = _Transformer(n_layers)


class Wav2Vec2Params(nn.Module):
    def __init__(self, n_layers=24):
        super().__init__()
        self.feature_extractor = _FeatureExtractor()
        self.encoder = _Encoder(n_layers)


def frames_out(n):
    for _, k, s in CONV_LAYERS:
        n = (n - k) // s + 1
    return n


def _polyphase_stride2_weight(w):
    """stride-2 conv weight [Cout, Cin, k] -> stride-1 weight over [even phase | odd phase] channels:
    out[t] = sum_j w[j] x[2t + j] = sum_m ( w[2m] x_even[t + m] + w[2m+1] x_odd[t + m] )"""
    cout, cin, k = w.shape
    kp = (k + 1) // 2
    wc = torch.zeros(cout, 2 * cin, kp, dtype=w.dtype, device=w.device)
    for j in range(k):
        wc[:, (j % 2) * cin:(j % 2 + 1) * cin, j // 2] = w[:, :, j]
    return wc, kp


class TdnnfWav2vec2VqNet(_TdnnfBase):
    def __init__(self, output_dim, hidden_dim=1024, bottleneck_dim=128, prefinal_bottleneck_dim=256,
                 kernel_size_list=([3, 3, 3], [1, 3, 3, 3]), subsampling_factor_list=([1, 1, 1], [1.5, 1, 1, 1]),
                 p_dropout=0.1, codebook_size=48):
        super().__init__()
        self.input_dim = 1024
        self.preprocessor = Wav2Vec2Params(24)
        self.output_dim = output_dim
        self.padding = get_padding(kernel_size_list[0], subsampling_factor_list[0]) // 2
        self.padding_after = get_padding(kernel_size_list[1], subsampling_factor_list[1]) // 2
        self.tdnn1, self.tdnnfs = tdnnf_stack(self.input_dim, hidden_dim, bottleneck_dim, prefinal_bottleneck_dim,
                                              kernel_size_list[0], subsampling_factor_list[0], codebook_size)
        _AsrHead.attach(self, hidden_dim, bottleneck_dim, prefinal_bottleneck_dim, kernel_size_list[1],
                        subsampling_factor_list[1], output_dim)
        self._init_cache()
        self._w2 = None
        self._w2_key = None

    # ---- kernel-ready weights of the wav2vec2 part -------------------------------------------
    #: arithmetic of the wav2vec2 matrix products (conv feature extractor after layer 0, feature projection,
    #: the 24 x 6 transformer Linear layers): "f16x3" (split-f16 on the f16 matrix cores, ~2^-21 relative per
    #: product; with it also the fused attention kernel and the positional conv as chained 11-tap pieces) or "f32"
    #: (exact f32 MFMA everywhere, attention as scores GEMM + softmax + apply GEMM).
    w2v2_precision = os.environ.get("SATOOLS_AMD_W2V2_PRECISION", "f16x3")
    #: the transformer's residual stream on a row pitch of round_up(T, 64) frames instead of T (same values; aligned 128-byte rows)
    residual_pitch = int(os.environ.get("SATOOLS_AMD_W2V2_PITCH", "1"))
    #: the feature extractor's stride-2 3-tap convs as one wrapped 1x1 product on the ring GEMM (0: two-tap polyphase conv)
    fe_wrapped_gemm = int(os.environ.get("SATOOLS_AMD_W2V2_FE_WRAPPED_GEMM", "1"))

    def _prepare_w2v2(self, device):
        if self.__dict__.get("_frozen"):           # packings installed by frozen.load_frozen: one per precision the file stores
            hit = self.__dict__.get("_w2_store", {}).get(self.w2v2_precision)
            if hit is None:
                raise _lib.SatError(f"frozen model: its file stores no {self.w2v2_precision!r} packing of the wav2vec2 encoder "
                                    "(export_frozen(..., exact_extractor=True) stores the exact-f32 one)")
            self._w2_key, self._w2, self._mm_mode = hit
            return self._w2
        key = (self.w2v2_precision,) + tuple((p.data_ptr(), p._version, str(p.device)) for p in self.preprocessor.parameters())
        if self._w2_key == key:
            return self._w2
        if self.w2v2_precision not in ("f16x3", "f32"):
            raise _lib.SatError(f"unknown wav2vec2 precision {self.w2v2_precision!r}")
        # one packing per precision is kept (asrbn._TdnnfBase._prepare: the near-tie guard switches to the exact kernels for single utterances)
        store = self.__dict__.setdefault("_w2_store", {})
        if self._w2_key is not None:
            store[self._w2_key[0]] = (self._w2_key, self._w2, self._mm_mode)
        hit = store.get(self.w2v2_precision)
        if hit is not None and hit[0] == key:
            self._w2_key, self._w2, self._mm_mode = hit
            return self._w2
        _lib.cache_rebuild_begin(device, hit is not None)
        split = self.w2v2_precision == "f16x3"
        pack_mm = packing.pack_conv_weight_f16x3 if split else packing.pack_conv_weight
        self._mm_mode = _lib.CONV_F16X3 if split else _lib.CONV_F32
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        pre = self.preprocessor
        W = {"fe": []}
        for i, blk in enumerate(pre.feature_extractor.conv_layers):
            w = f32(blk.conv.weight)
            ent = {"b": f32(blk.conv.bias), "g": f32(blk.layer_norm.weight), "beta": f32(blk.layer_norm.bias)}
            if i == 0:
                ent["w"] = w.reshape(w.shape[0], w.shape[2]).contiguous()       # [512][10]
            else:
                wc, kp = _polyphase_stride2_weight(w)
                ent["w"], ent["k"] = pack_mm(wc), kp
                if split and w.shape[2] == 3 and self.fe_wrapped_gemm:
                    # 3 taps, stride 2 on [even | odd] planes as ONE product over 3 C input channels, the last C of them
                    # (tap 2) reading the even phase one frame later (sat_conv1d_desc.x_wrap_channels): no zero tap
                    ent["w_wrap"] = pack_mm(torch.cat([w[:, :, 0], w[:, :, 1], w[:, :, 2]], 1).unsqueeze(-1).contiguous())
            W["fe"].append(ent)
        fp = pre.encoder.feature_projection
        W["fp"] = {"g": f32(fp.layer_norm.weight), "beta": f32(fp.layer_norm.bias),
                   "w": pack_mm(f32(fp.projection.weight).unsqueeze(-1)), "b": f32(fp.projection.bias)}
        tr = pre.encoder.transformer
        pc = tr.pos_conv_embed.conv
        wv, wg = f32(pc.weight_v), f32(pc.weight_g)
        wpos = torch._weight_norm(wv, wg, 2)                                      # weight_norm(dim=2)
        W["pos"] = {"w": packing.pack_conv_weight(wpos, groups=16), "b": f32(pc.bias)}
        if self._mm_mode == _lib.CONV_F16X3:
            # split-f16: the 128 taps as twelve 11-tap grouped convs over shifted windows, chained through the
            # pre-activation residual (the split-f16 kernels are instantiated for 11 taps, not for 128)
            W["pos"]["pieces"] = []
            for s_ in range(12):
                ws = torch.zeros(wpos.shape[0], wpos.shape[1], 11, dtype=torch.float32, device=wpos.device)
                n_ = min(11, wpos.shape[2] - 11 * s_)
                ws[:, :, :n_] = wpos[:, :, 11 * s_:11 * s_ + n_]
                W["pos"]["pieces"].append(packing.pack_conv_weight_f16x3(ws, groups=16))
        W["layers"] = []
        for lay in tr.layers:
            at = lay.attention
            W["layers"].append({
                "ln1": (f32(lay.layer_norm.weight), f32(lay.layer_norm.bias)),
                "q_w": pack_mm(f32(at.q_proj.weight).unsqueeze(-1)), "q_b": f32(at.q_proj.bias),
                "k_w": pack_mm(f32(at.k_proj.weight).unsqueeze(-1)), "k_b": f32(at.k_proj.bias),
                "v_w": pack_mm(f32(at.v_proj.weight).unsqueeze(-1)), "v_b": f32(at.v_proj.bias),
                "o_w": pack_mm(f32(at.out_proj.weight).unsqueeze(-1)), "o_b": f32(at.out_proj.bias),
                "ln2": (f32(lay.final_layer_norm.weight), f32(lay.final_layer_norm.bias)),
                "f1_w": pack_mm(f32(lay.feed_forward.intermediate_dense.weight).unsqueeze(-1)),
                "f1_b": f32(lay.feed_forward.intermediate_dense.bias),
                "f2_w": pack_mm(f32(lay.feed_forward.output_dense.weight).unsqueeze(-1)),
                "f2_b": f32(lay.feed_forward.output_dense.bias),
            })
        self._w2, self._w2_key = W, key
        _lib.cache_rebuild_end(device)
        return W

    # ---- wav2vec2 forward: [B, n] -> last layer output [B, 1024, frames] ------------------------
    def w2v2_features(self, wav, hook=None):
        """`hook(name, f32 tensor or None, planes or None)`, if given, sees the intermediates (the mirror of oracle.convert.forward's
        `hook`): "ln0" (conv 0 + its LayerNorm), "conv1" / "ln1" .. "conv6" / "ln6", "proj", "pos" (the input of layer 0), "last".  A
        stage that hands on split planes only passes None for the f32 tensor; the LayerNorms before a stride-2 conv pass their
        phase-split form.  No launch depends on it."""
        W = self._prepare_w2v2(wav.device)
        mm = self._mm_mode
        B, n = wav.shape
        fe_len = self._fe_lens(n)       # (from THIS call's length: a field set by features() went stale when another call — the tie
                                        # guard's calibration utterances, a flagged row decided again — ran in between)
        heads, hd = 16, 64
        # conv feature extractor
        planes = mm == _lib.CONV_F16X3        # split-f16: LayerNorm hands its result on as split planes (16-byte staging)
        x = None if planes else ops.w2v2_conv0(wav, W["fe"][0]["w"], W["fe"][0]["b"])   # [B, 512, T0]
        for i in range(7):
            e = W["fe"][i]
            last = i == 6
            # LayerNorm over channels + GELU; for a following stride-2 conv the output is phase-split
            if planes and i == 0:
                # conv layer 0 and its LayerNorm in one kernel: the [B, 512, 16k] f32 tensor (1 GB) never exists
                x, xs = ops.w2v2_conv0_ln(wav, e["w"], e["b"], e["g"], e["beta"])
            elif planes and not last:
                x, xs = ops.layernorm_ch(x, e["g"], e["beta"], gelu=True, split_phases=True, planes=True, want_f32=False)
            else:
                x, xs = ops.layernorm_ch(x, e["g"], e["beta"], gelu=True, split_phases=not last), None
            if hook:
                hook(f"ln{i}", None if xs is not None else x, xs)
            if not last:
                nxt = W["fe"][i + 1]
                if xs is not None and "w_wrap" in nxt:
                    x = ops.conv1d(x, nxt["w_wrap"], 512, 1, bias=nxt["b"], t_out=fe_len[i + 1], mode=mm, x_split=xs,
                                   x_wrap_channels=x.shape[1], c_in=3 * x.shape[1] // 2)
                else:
                    x = ops.conv1d(x, nxt["w"], 512, nxt["k"], bias=nxt["b"], pad_left=0, pad_right=0, t_out=fe_len[i + 1], mode=mm,
                                   x_split=xs)
                if hook:
                    hook(f"conv{i + 1}", x, None)
        T = x.shape[2]
        # feature projection
        if planes:
            x, xs = ops.layernorm_ch(x, W["fp"]["g"], W["fp"]["beta"], planes=True, want_f32=False)
        else:
            x, xs = ops.layernorm_ch(x, W["fp"]["g"], W["fp"]["beta"]), None
        x = ops.conv1d(x, W["fp"]["w"], 1024, 1, bias=W["fp"]["b"], mode=mm, x_split=xs)
        if hook:
            hook("proj", x, None)
        # positional conv (grouped, k = 128, pad 64, last sample dropped) + GELU, added to x
        if "pieces" in W["pos"]:
            y = None
            for s_, wsp in enumerate(W["pos"]["pieces"]):
                pl = 64 - 11 * s_           # taps 11 s .. 11 s + 10 of the 128 (pad 64): a window shifted by 11 s
                y = ops.conv1d(x, wsp, 1024, 11, bias=W["pos"]["b"] if s_ == 0 else None, pad_left=pl, pad_right=10 - pl,
                               groups=16, mode=mm, res=y, gelu=(s_ == 11), out=y)
            x = ops.add3(y, x)
        else:
            x = ops.conv1d(x, W["pos"]["w"], 1024, 128, bias=W["pos"]["b"], pad_left=64, pad_right=63, groups=16,
                           gelu=True, post_res=x)
        if hook:
            hook("pos", x, None)
        # NO encoder-level LayerNorm here: torchaudio builds Transformer(layer_norm_first=not encoder_layer_norm_first),
        # so `encoder.transformer.layer_norm` runs after the stack in forward() and not at all in
        # get_intermediate_outputs / extract_features, whose [-1] the reference takes (tdnnf_wav2vec2_vq.py:295-297);
        # cross-checked against HF transformers (tests/golden/make_w2v2_crosscheck.py).  The parameter stays in the
        # state dict, unused on this path.
        G = B * heads
        tp = ((T + 63) // 64) * 64   # row pitch of the per-head tensors = the packed-weight co_pad for T rows
        # Linear layers read their input as split planes (16-byte staging, two 16-channel sub-chunks per pipeline
        # stage): 182 -> ~60 us per layer
        sp = (lambda t: ops.act_split(t, 1.0)) if planes else (lambda t: None)
        ln = (lambda t, p: ops.layernorm_ch(t, *p, planes=True, want_f32=False)) if planes else (lambda t, p: (ops.layernorm_ch(t, *p), None))
        # The residual stream x lives in two buffers of row pitch tp (a multiple of 64 frames: 249 -> 256), written alternately by the
        # two residual GEMMs of a layer: with the natural pitch of 249 floats no row starts on a 128-byte line, and every 128-byte
        # piece the LayerNorm and the GEMM epilogues read or write straddles two (SATOOLS_AMD_W2V2_PITCH=0: the contiguous form)
        pitched = planes and self.residual_pitch
        if pitched:
            xbuf = [torch.empty(B, 1024, tp, dtype=torch.float32, device=x.device) for _ in range(2)]
            xbuf[0][:, :, :T].copy_(x)
            x = xbuf[0][:, :, :T]
        nb = 1
        for L in W["layers"]:
            h, hs = ln(x, L["ln1"])
            v = torch.empty(B, 1024, tp, dtype=torch.float32, device=x.device)
            if planes:
                # fused attention (csrc/w2v2.hip): Q and K leave their projections as split planes, the scores stay
                # in registers, the context comes back as planes for the output projection
                qs, ks = ops.split_like(B, 1024, T, x.device), ops.split_like(B, 1024, T, x.device)
                # q | k | v: three GEMMs of one shape on the same input — one launch of the persistent ring (sat_conv1d_multi_f32)
                ops.conv1d_multi([
                    (h, L["q_w"], 1024, 1, dict(bias=L["q_b"], mode=mm, x_split=hs, y_split=qs, y_split_slope=1.0, no_y=True)),
                    (h, L["k_w"], 1024, 1, dict(bias=L["k_b"], mode=mm, x_split=hs, y_split=ks, y_split_slope=1.0, no_y=True)),
                    (h, L["v_w"], 1024, 1, dict(bias=L["v_b"], out=v[:, :, :T], mode=mm, x_split=hs))])
                o, os_ = ops.attention_fused(qs, ks, v, B, heads, hd, T, hd ** -0.5)
                x = ops.conv1d(o, L["o_w"], 1024, 1, bias=L["o_b"], res=x, mode=mm, x_split=os_, out=xbuf[nb][:, :, :T] if pitched else None)
                nb ^= 1
            else:
                q = torch.empty(B, 1024, tp, dtype=torch.float32, device=x.device)
                k = torch.empty_like(q)
                ops.conv1d(h, L["q_w"], 1024, 1, bias=L["q_b"], out=q[:, :, :T], mode=mm, x_split=hs)
                ops.conv1d(h, L["k_w"], 1024, 1, bias=L["k_b"], out=k[:, :, :T], mode=mm, x_split=hs)
                ops.conv1d(h, L["v_w"], 1024, 1, bias=L["v_b"], out=v[:, :, :T], mode=mm, x_split=hs)
                # S^T[j][q] = sum_c K[c][j] Q[c][q]  per (utterance, head): K as packed weights, Q as input
                st = torch.empty(G * T, tp, dtype=torch.float32, device=x.device)
                ops.attention_scores(q, k, st, B, heads, hd, T)
                ops.softmax_cols(st, G, T, scale=hd ** -0.5)
                vt = ops.transpose_heads(v, B, heads, hd, T)                           # [G][jpad][64]
                o = ops.attention_apply(st, vt, B, heads, hd, T)                        # [B, 1024, T]
                x = ops.conv1d(o, L["o_w"], 1024, 1, bias=L["o_b"], res=x, mode=mm)
            h, hs = ln(x, L["ln2"])
            if planes:
                fs = ops.split_like(B, 4096, T, x.device)
                f = ops.conv1d(h, L["f1_w"], 4096, 1, bias=L["f1_b"], gelu=True, mode=mm, x_split=hs, y_split=fs,
                               y_split_slope=1.0, no_y=True)                        # f: shape carrier only
                x = ops.conv1d(f, L["f2_w"], 1024, 1, bias=L["f2_b"], res=x, mode=mm, x_split=fs, out=xbuf[nb][:, :, :T] if pitched else None)
                nb ^= 1
            else:
                h = ops.conv1d(h, L["f1_w"], 4096, 1, bias=L["f1_b"], gelu=True, mode=mm)
                x = ops.conv1d(h, L["f2_w"], 1024, 1, bias=L["f2_b"], res=x, mode=mm)
        if hook:
            hook("last", x, None)
        return x

    @staticmethod
    def _fe_lens(n):
        """frames after each of the seven conv layers of the feature extractor for n samples"""
        lens, t = [], n
        for _, k, s in CONV_LAYERS:
            t = (t - k) // s + 1
            lens.append(t)
        return lens

    def features(self, x):
        """[N, n] raw waveforms -> [N, 1024, 250 + 2 * padding]: last transformer layer output, replicate-padded by one
        frame (249 -> 250), then pad_input(self.padding)   (tdnnf_wav2vec2_vq.py:295-306 == :320-331)"""
        if not x.is_cuda:
            raise _lib.SatError("the wav2vec2 extractor runs on the HIP device only (no CPU fallback); move the input to 'cuda'")
        if x.dim() != 2:
            raise _lib.SatError("expected a 2-dimensional tensor [N, samples]")
        if self._fe_lens(x.shape[1])[-1] < 1:
            raise _lib.SatError("input too short for the wav2vec2 feature extractor")
        feats = self.w2v2_features(x.to(torch.float32).contiguous())                # [N, 1024, 249]
        feats = ops.pad_replicate(feats, 0, 1)                                      # F.pad(.., (0, 1), "replicate")
        return ops.pad_replicate(feats, self.padding, self.padding, interleave_right=True)   # pad_input

    def _extract_bn_private(self, x, defer_ties=False):
        with self._lock():
            return self._bn_guarded(self.features(x), x, defer_ties)            # this tag never mutates its input

    def _features_of(self, x):
        return self.features(x)

    def _exact_stored(self):
        return super()._exact_stored() and (not self.__dict__.get("_frozen") or "f32" in self.__dict__.get("_w2_store", {}))

    def _exact_rows(self, rows, feats, wav, spans=None):
        """flagged utterances again on the exact-f32 kernels: the encoder is recomputed for those rows; their frames and their own
        replicated frames (left pad, the 250th frame) replace the split-f16 ones in a copy of the batch's padded features, the
        right-hand pad frames — `pad_input` tiles the last frames of ALL utterances of the batch there (tdnnf_vq.py:228-234) — stay the
        batch's (another row's frames are not recomputed)"""
        with self._exact(self):
            f = self.w2v2_features(wav[rows].to(torch.float32).contiguous())      # [n, 1024, 249]
            sub = feats[rows].contiguous()
            p, T = self.padding, f.shape[2]
            sub[:, :, p:p + T] = f
            sub[:, :, p + T] = f[:, :, -1]
            sub[:, :, :p] = f[:, :, :1]
            # (the whole utterance: attention and the positional conv look at every frame — `spans` is not used on this tag)
            zq, (_, idx_x, _) = self._run_stack(sub, want_aux=True)
            return zq, idx_x, [0] * len(rows)

    def extract_bn(self, x: torch.Tensor, want_aux=False) -> torch.Tensor:
        """inputs [N, n] in [-1, 1] (no 32768 scaling on this tag) -> [N, T, 256]
        (tdnnf_wav2vec2_vq.py:289-314)"""
        if want_aux:                           # diagnostics: the arithmetic as configured, no second decision
            out = self._run_stack(self.features(x), want_aux=True)
            return out[0].permute(0, 2, 1), out[1]
        with self._lock():
            return self._bn_guarded(self.features(x), x)

    def forward(self, x):
        """waveforms [N, n] in [-1, 1] -> (chain_out, log_softmax(xent_out)), each [N, T', output_dim]
        (tdnnf_wav2vec2_vq.py:316-345, eval mode): the wav2vec2 features through tdnn1, the TDNNF
        layers with the VQ layer run through, pad_input(padding_after), tdnnfs_after (1.5x subsampling first),
        the two prefinal layers and the output affines — the boundary to the Kaldi decoder"""
        return self._asr_outputs(self.features(x))


class TdnnfWav2vec2Net(TdnnfWav2vec2VqNet):
    """wav2vec2-large front end + TDNNF tail, no quantiser (tdnnf_wav2vec2.py:21-285; the wav2vec2 *_aug tag): no
    `bottleneck_func.*` entries in the state dict, `extract_bn` returns linearB's 256-dim output (tdnnf_wav2vec2.py:221-243),
    no near-tie guard."""

    def __init__(self, output_dim, hidden_dim=1024, bottleneck_dim=128, prefinal_bottleneck_dim=256,
                 kernel_size_list=([3, 3, 3], [1, 3, 3, 3]), subsampling_factor_list=([1, 1, 1], [1.5, 1, 1, 1]), p_dropout=0.1):
        super().__init__(output_dim, hidden_dim, bottleneck_dim, prefinal_bottleneck_dim, kernel_size_list, subsampling_factor_list,
                         p_dropout, codebook_size=None)
