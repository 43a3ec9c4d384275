"""ASV x-vector extractor (half-ResNet34 with squeeze-excitation) behind the reference's `Net` interface
(reference: egs/asv/voxceleb/local/tuning/resnet.py:17-79 — the `asv_eval_vox1_resnet` model the anonymization recipe evaluates with):
`model(wav)` returns `((loss, logits), x_vector)` like the reference's forward with `target=None` — loss = NaN, logits = None, the
L2-normalised 256-dim embedding — computed on the HIP kernels:

  front end   the ECAPA net's (xvector.py): log-mel + InstanceNorm                    csrc/xvector.hip, bodies in csrc/xvector_tile.h
  ResNet      37 Conv2d + BatchNorm2d(eval) (+ ReLU): exact f32 MFMA implicit GEMM      csrc/conv2d.hip  conv2d_mfma_kernel, conv2d_stem_kernel
              opt-in (`conv2d_precision = "f16x3"`): the 36 convs of the blocks in        csrc/conv2d16/   conv2d_f16x3_kernel
              split-f16 arithmetic, exact f32 again for a batch that leaves the f16 range
              SE squeeze (mean over H x W), its two Linear layers                       row_mean_rows_kernel, linear_rows_kernel
              relu(out * sigmoid(gate) + shortcut)                                      se_scale_add_relu_kernel
  pooling     global context: mean / unbiased std over time                             row_mean_std_kernel
              attention MLP (1x1 Conv1d on the fused conv kernel), tanh                 conv1d, tanh_kernel
              softmax over time + weighted mean / std at C = 2560                       attentive_stats_kernel
  head        Linear(5120 -> 256) + BatchNorm, L2 norm                                  linear_rows_kernel, l2norm_rows_kernel
  ragged      `extract_batch`: utterances of unequal length side by side on one       csrc/ragged2d/resnet_ragged.hip, the segment forms of
              packed time axis per time resolution, exact f32                          the conv, the squeeze, the tail and the context
              opt-in (`ragged_conv2d_precision = "f16x3"`): the 36 block convs in         csrc/ragged2d16/  conv2d_segments_f16x3_kernel
              split-f16 arithmetic, exact f32 again for the utterances that leave the f16 range

AXES.  The reference runs the ResNet on [B, 1, T, 80] images, frequency innermost (sidekit/archi.py:110-113), and permutes its
[B, 256, T', 10] output to [B, 2560, T'] for the pooling (sidekit/pooling.py:126-128).  Here TIME stays innermost from the front end's
[B, 80, T] to the pooling: a 3x3 conv commutes with transposing both the image and the kernel, so `_prepare` packs every 3x3 weight with
its two kernel axes swapped, and the last layer's [B, 256, 10, T'] output is the pooling's input without a copy.

The parameter tree carries the reference's state-dict keys and shapes, so a reference checkpoint loads with `load_state_dict`.
No CPU fallback.  An utterance with fewer than two pooled frames (T' < 2: under 9 front-end frames, 1 280 samples) is refused with
SatError: the reference's global context takes the UNBIASED deviation over T' (torch.std), which is NaN there."""
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib, ops, packing
from .xvector import _ArcMargin, _MelSpecFrontEnd

BLOCKS = (3, 4, 6, 3)
PLANES = (32, 64, 128, 256)


class _SELayer(nn.Module):
    def __init__(self, channel, reduction=16):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction, bias=False), nn.ReLU(inplace=True),
                                nn.Linear(channel // reduction, channel, bias=False), nn.Sigmoid())


class _BasicBlock(nn.Module):
    def __init__(self, in_planes, planes, stride, shortcut):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.se = _SELayer(planes)
        self.shortcut = nn.Sequential()
        if shortcut:
            self.shortcut = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=stride, bias=False), nn.BatchNorm2d(planes))


class _PreHalfResNet34(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, PLANES[0], 3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(PLANES[0])
        in_planes = PLANES[0]
        for i, (planes, n) in enumerate(zip(PLANES, BLOCKS)):
            blocks = []
            for j in range(n):
                # the reference's make_layer hands the FIRST block of every layer its stride as a tuple, and ResNetBasicBlock tests
                # `stride != 1` (sidekit/nn.py:50): true for (1, 1) as well, so layer1's first block has a 1x1 stride-1 shortcut too
                blocks.append(_BasicBlock(in_planes, planes, 2 if (i > 0 and j == 0) else 1, shortcut=j == 0))
                in_planes = planes
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))


class _AttentivePooling(nn.Module):
    def __init__(self, num_channels, num_freqs=10, attention_channels=128):
        super().__init__()
        d = num_channels * num_freqs
        self.attention = nn.Sequential(nn.Conv1d(3 * d, attention_channels, 1), nn.ReLU(), nn.BatchNorm1d(attention_channels), nn.Tanh(),
                                       nn.Conv1d(attention_channels, d, 1), nn.Softmax(dim=2))


def pooled_frames(frames):
    """front-end frames -> frames the pooling sees: three stride-2 layers, each (n - 1) // 2 + 1"""
    for _ in range(3):
        frames = (frames - 1) // 2 + 1
    return frames


def build(args=None):
    """same contract as the reference's model-config `build(args)`: returns the Net class"""

    class Net(nn.Module):
        #: arithmetic of the attention's two 1x1 convs: "f16x3" (split-f16 on the f16 matrix cores) or "f32" (exact f32 MFMA); the 2-D
        #: convs are governed by `conv2d_precision` alone
        precision = os.environ.get("SATOOLS_AMD_XVECTOR_PRECISION", "f16x3")
        #: arithmetic of the 2-D convs of the residual blocks (3x3 and 1x1 shortcuts): "f32" (exact f32 MFMA, the default) or "f16x3"
        #: (split-f16, csrc/conv2d16/).  The stem is exact f32 either way.  A batch with an activation outside the f16 range
        #: (|x| >= 65 520 or non-finite) is run again in "f32": `split_fallbacks` counts those, `last_conv2d_arithmetic` names what the
        #: last batch's result came from
        conv2d_precision = os.environ.get("SATOOLS_AMD_RESNET_CONV2D", "f32")
        #: arithmetic of the same convs in a RAGGED call (`extract_batch`), which `conv2d_precision` does not govern: "f32" (the default) or
        #: "f16x3" (split-f16 on the packed time axis, csrc/ragged2d16/).  An utterance with an activation outside the f16 range is extracted
        #: again in "f32", alone among its batch: `last_split_fallback_rows` names those of the last ragged call, `split_fallbacks` counts
        #: the calls that had any, `last_conv2d_arithmetic` is then "f16x3+f32" ("f32" if every row fell back)
        ragged_conv2d_precision = os.environ.get("SATOOLS_AMD_RESNET_CONV2D_RAGGED", "f32")
        split_fallbacks = 0
        last_conv2d_arithmetic = None
        last_split_fallback_rows = None

        def __init__(self, num_speakers=1):
            super().__init__()
            self.preprocessor = _MelSpecFrontEnd()
            self.sequence_network = _PreHalfResNet34()
            self.embedding_size = 256
            self.before_speaker_embedding = nn.Sequential(OrderedDict([
                ("lin_be", nn.Linear(5120, self.embedding_size, bias=False)), ("bn_be", nn.BatchNorm1d(self.embedding_size))]))
            self.stat_pooling = _AttentivePooling(256, 10)
            self.after_speaker_embedding = _ArcMargin(self.embedding_size, num_speakers)
            self._cache, self._cache_key, self._mel_ranges = None, None, None
            super().eval()

        def train(self, mode=True):
            if mode:
                raise _lib.SatError("the MI355X x-vector extractor is inference only")
            return super().train(False)

        # ---- kernel-ready weights ----------------------------------------------------------------
        def _prepare(self, device):
            if self.conv2d_precision not in ("f32", "f16x3"):
                raise _lib.SatError(f"conv2d_precision = {self.conv2d_precision!r}: \"f32\" or \"f16x3\"")
            if self.ragged_conv2d_precision not in ("f32", "f16x3"):
                raise _lib.SatError(f"ragged_conv2d_precision = {self.ragged_conv2d_precision!r}: \"f32\" or \"f16x3\"")
            key = (self.precision, self.conv2d_precision, self.ragged_conv2d_precision) + tuple((p.data_ptr(), p._version, str(p.device)) for p in list(self.parameters()) + list(self.buffers()))
            if self._cache_key == key:
                return self._cache
            _lib.cache_rebuild_begin(device, self._cache is not None)
            f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
            split = self.precision == "f16x3"
            pack1 = packing.pack_conv_weight_f16x3 if split else packing.pack_conv_weight

            def bn_affine(bn):
                s = f32(bn.weight) / torch.sqrt(f32(bn.running_var) + bn.eps)
                return s.contiguous(), (f32(bn.bias) - f32(bn.running_mean) * s).contiguous()

            split2d = self.conv2d_precision == "f16x3"
            ragged16 = self.ragged_conv2d_precision == "f16x3"

            def cb(conv, bn, stem=False):
                # the kernel axes swapped: this net keeps time innermost, the reference frequency (module docstring)
                sc, sh = bn_affine(bn)
                e = {"w": ops.pack_conv2d_weight(f32(conv.weight), transpose=True), "k": conv.kernel_size[0], "s": conv.stride[0], "scale": sc, "shift": sh}
                if (split2d or ragged16) and not stem:
                    # (the exact-f32 packing stays: a batch or an utterance that leaves the f16 range runs on it)
                    e["w16"], e["descale"] = ops.pack_conv2d_weight_f16x3(f32(conv.weight), transpose=True)
                return e

            sn = self.sequence_network
            W = {"stem": cb(sn.conv1, sn.bn1, stem=True), "blocks": [], "split2d": split2d, "ragged16": ragged16}
            for i in range(4):
                for blk in getattr(sn, f"layer{i + 1}"):
                    W["blocks"].append({"c1": cb(blk.conv1, blk.bn1), "c2": cb(blk.conv2, blk.bn2),
                                        "fc0": f32(blk.se.fc[0].weight), "fc2": f32(blk.se.fc[2].weight),
                                        "sc": cb(blk.shortcut[0], blk.shortcut[1]) if len(blk.shortcut) else None})
            att = self.stat_pooling.attention
            d = att[4].weight.shape[0]                                            # 2560
            w0 = f32(att[0].weight)                                               # [128, 3 d, 1]: frames, context mean, context std
            sc, sh = bn_affine(att[2])
            W["att1"] = {"w": pack1(w0[:, :d].contiguous()), "w_ctx": w0[:, d:, 0].contiguous(), "b": f32(att[0].bias), "scale": sc, "shift": sh,
                         "cout": w0.shape[0]}
            W["att2"] = {"w": pack1(f32(att[4].weight)), "b": f32(att[4].bias), "cout": d}
            W["mode1"] = _lib.CONV_F16X3 if split else _lib.CONV_F32
            sc, sh = bn_affine(self.before_speaker_embedding.bn_be)
            W["emb"] = {"w": f32(self.before_speaker_embedding.lin_be.weight), "scale": sc, "shift": sh}
            W["window"] = f32(self.preprocessor.MelSpec.spectrogram.window)
            W["fb"] = f32(self.preprocessor.MelSpec.mel_scale.fb).t().contiguous()      # [80][513]
            W["coef"] = float(-self.preprocessor.PreEmphasis.flipped_filter.reshape(-1)[0])
            self._cache, self._cache_key = W, key
            _lib.cache_rebuild_end(device)
            return W

        # ---- forward -----------------------------------------------------------------------------
        def features(self, x):
            """[B, n] -> [B, 80, 1 + n // 160]: log-mel front end + InstanceNorm (sidekit/preprocessor.py:223-236)"""
            W = self._prepare(x.device)
            return ops.instnorm_rows(ops.melspec_logmel(x, W["window"], W["fb"], W["coef"]))

        @staticmethod
        def _conv(x, e, relu=False, flag=None):
            """`flag` (the batch's int32 overflow flag) selects the split-f16 form"""
            if flag is not None:
                return ops.conv2d_f16x3(x, e["w16"], e["descale"], e["k"], e["s"], ch_scale=e["scale"], ch_shift=e["shift"], relu=relu, overflow=flag)
            return ops.conv2d(x, e["w"], e["k"], e["s"], ch_scale=e["scale"], ch_shift=e["shift"], relu=relu)

        def _block(self, x, blk, flag=None):
            """ResNetBasicBlock.forward (sidekit/nn.py:57-68) with SELayer.forward (nn.py:23-32)"""
            out = self._conv(self._conv(x, blk["c1"], relu=True, flag=flag), blk["c2"], flag=flag)
            B, C = out.shape[:2]
            m = ops.row_mean(out.view(B, C, -1))                                    # [B, C, 1]
            g = ops.linear_rows(ops.linear_rows(m, blk["fc0"], relu=True), blk["fc2"])      # the gate's logits
            r = x if blk["sc"] is None else self._conv(x, blk["sc"], flag=flag)
            return ops.se_scale_add_relu(out, g, r)

        def resnet(self, feats, taps=None):
            """[B, 80, T] -> [B, 256, 10, T']; `taps` (a dict) receives the stem's output and each layer's, for the tests"""
            W = self._prepare(feats.device)
            stem = self._conv(feats.unsqueeze(1), W["stem"], relu=True)
            if taps is not None:
                taps["bn1"] = stem

            def blocks(flag):
                x, i = stem, 0
                for li, n in enumerate(BLOCKS):
                    for _ in range(n):
                        x = self._block(x, W["blocks"][i], flag)
                        i += 1
                    if taps is not None:
                        taps[f"layer{li + 1}"] = x
                return x

            if W["split2d"]:
                # one zeroed flag per batch (its own allocation: batches on other streams have theirs), read once after the last block
                flag = torch.zeros(1, dtype=torch.int32, device=feats.device)
                x = blocks(flag)
                if int(flag.item()) == 0:
                    self.last_conv2d_arithmetic = "f16x3"
                    return x
                self.split_fallbacks += 1                                         # an activation left the f16 range: exact f32 for this batch
            self.last_conv2d_arithmetic = "f32"
            return blocks(None)

        def pool(self, x, taps=None):
            """AttentivePooling(256, 10, global_context=True).forward (sidekit/pooling.py:118-138): [B, 2560, T'] -> [B, 5120, 1].
            The context's 5120 channels are constant over time: their share of the first conv is one matrix-vector product per
            utterance, added to the frames' 2560 -> 128 product before the ReLU"""
            W = self._prepare(x.device)
            B, d, t = x.shape
            a1, a2 = W["att1"], W["att2"]
            gc = ops.row_mean_std(x)                                                                # [B, 5120]
            ctx = ops.linear_rows(gc, a1["w_ctx"], bias=a1["b"])                                    # [B, 128]
            a = ops.conv1d(x, a1["w"], a1["cout"], 1, res=ctx.unsqueeze(2).expand(B, a1["cout"], t).contiguous(), relu=True, relu_first=True,
                           ch_scale=a1["scale"], ch_shift=a1["shift"], mode=W["mode1"])
            logits = ops.conv1d(ops.tanh_(a), a2["w"], a2["cout"], 1, bias=a2["b"], mode=W["mode1"])
            if taps is not None:
                taps.update(gc=gc, a=a, logits=logits)
            return ops.attentive_stats(x, logits)

        def embed(self, feats, taps=None):
            W = self._prepare(feats.device)
            B, _, frames = feats.shape
            if pooled_frames(frames) < 2:
                raise _lib.SatError(f"x-vector extraction: {frames} frames leave {pooled_frames(frames)} pooled frame; the global context's unbiased "
                                    "deviation needs two (the reference returns NaN here)")
            x = self.resnet(feats, taps)
            pooled = self.pool(x.view(B, x.shape[1] * x.shape[2], x.shape[3]))
            if taps is not None:
                taps["pooled"] = pooled
            e = ops.linear_rows(pooled, W["emb"]["w"], ch_scale=W["emb"]["scale"], ch_shift=W["emb"]["shift"])
            return ops.l2norm_rows(e.reshape(B, self.embedding_size))

        # ---- ragged batches (csrc/ragged2d/, include/satools_hip_ragged2d.h) ------------------------------
        @staticmethod
        def _conv_segments(x, e, tab_in, tab_out, relu=False, flags=None):
            """`flags` (the call's int32 overflow flags, one per utterance) selects the split-f16 form"""
            if flags is not None:
                return ops.conv2d_f16x3_segments(x, e["w16"], e["descale"], e["k"], e["s"], tab_in, tab_out, ch_scale=e["scale"], ch_shift=e["shift"],
                                                 relu=relu, overflow=flags)
            return ops.conv2d_segments(x, e["w"], e["k"], e["s"], tab_in, tab_out, ch_scale=e["scale"], ch_shift=e["shift"], relu=relu)

        def _block_segments(self, x, blk, tab_in, tab_out, flags=None):
            """`_block` on the packed images: conv1 and the shortcut go from the input's level to the output's (the same one at stride 1),
            conv2, the squeeze and the tail stay on the output's; the SE layer's two Linear layers see [B, C] rows as in `_block`"""
            out = self._conv_segments(self._conv_segments(x, blk["c1"], tab_in, tab_out, relu=True, flags=flags), blk["c2"], tab_out, tab_out, flags=flags)
            m = ops.plane_mean_segments(out, tab_out)                               # [B, C]
            g = ops.linear_rows(ops.linear_rows(m, blk["fc0"], relu=True), blk["fc2"])
            r = x if blk["sc"] is None else self._conv_segments(x, blk["sc"], tab_in, tab_out, flags=flags)
            return ops.se_scale_add_relu_segments(out, g, r, tab_out)

        def embed_segments(self, feats, levels, overflow=None):
            """`embed` of a packed feature tensor [1, 80, T_tot_0] -> [B, 256]; `levels` = the batch's ops.RaggedLevels.  The 2-D convs
            run in exact f32 (csrc/ragged2d/) unless `overflow` is given: an int32 tensor of B elements on the device, zeroed by the
            caller, with which the 36 block convs run in split-f16 arithmetic (csrc/ragged2d16/; `ragged_conv2d_precision` must be
            "f16x3", which packs their weights).  Element i is nonzero afterwards if an activation of utterance i left the f16 range: row i
            is then unspecified and the caller replaces it (`extract_batch` does); every other row is unaffected.  The stem is exact f32
            either way.  Gap columns of every intermediate hold anything: the segment kernels never read them, and the attention's 1x1
            convs are pointwise in time."""
            W = self._prepare(feats.device)
            if overflow is not None and not W["ragged16"]:
                raise _lib.SatError("embed_segments: overflow flags select the split-f16 convs, which need ragged_conv2d_precision = \"f16x3\"")
            self.last_conv2d_arithmetic = "f32" if overflow is None else "f16x3"
            x = self._conv_segments(feats.view(1, 1, feats.shape[-2], feats.shape[-1]), W["stem"], levels[0], levels[0], relu=True)
            i, lvl = 0, 0
            for li, n in enumerate(BLOCKS):
                for j in range(n):
                    nxt = lvl + 1 if (li > 0 and j == 0) else lvl
                    x = self._block_segments(x, W["blocks"][i], levels[lvl], levels[nxt], overflow)
                    i, lvl = i + 1, nxt
            tab = levels[lvl]
            x = x.view(1, x.shape[1] * x.shape[2], x.shape[3])                     # [1, 2560, T_tot_3]
            a1, a2 = W["att1"], W["att2"]
            gc = ops.row_mean_std_segments(x, tab)                                  # [B, 5120]
            ctx = ops.linear_rows(gc, a1["w_ctx"], bias=a1["b"])                    # [B, 128]
            # the context's share of every column: its utterance's row (a gap column takes some row; nothing reads it)
            res = ctx.index_select(0, levels.columns).t().contiguous().unsqueeze(0)         # [1, 128, T_tot_3]
            a = ops.conv1d(x, a1["w"], a1["cout"], 1, res=res, relu=True, relu_first=True, ch_scale=a1["scale"], ch_shift=a1["shift"], mode=W["mode1"])
            logits = ops.conv1d(ops.tanh_(a), a2["w"], a2["cout"], 1, bias=a2["b"], mode=W["mode1"])
            pooled = ops.attentive_stats_segments(x, logits, tab)                  # [B, 5120]
            # A NaN or an infinity among an utterance's samples makes its whole feature segment NaN (the InstanceNorm's mean), and the
            # reference's ReLU would carry that to the x-vector.  The conv epilogue's ReLU is max(v, 0), which gives 0 for NaN: the NaNs
            # would end after the stem.  So the segment's NaN is carried past the body as xvector.Net.embed_segments does:
            # 0 * (sum of the feature rows' means) is 0 for a finite segment and NaN otherwise, added to the pooled row.
            pooled = pooled + ops.row_mean_segments(feats, levels[0]).sum(1, keepdim=True) * 0.0
            e = ops.linear_rows(pooled, W["emb"]["w"], ch_scale=W["emb"]["scale"], ch_shift=W["emb"]["shift"])
            return ops.l2norm_rows(e)

        def extract_batch(self, wavs):
            """x-vectors of a RAGGED batch in one launch sequence: `wavs` = a list of 1-D device tensors of any lengths, or
            (padded [B, n_max], lengths) with anything past each length and `lengths` a list or a CPU tensor -> [B, 256], row i the
            L2-normalised x-vector of utterance i at its own length (what `forward` gives for it alone, to f32 rounding) — and all NaN for
            an utterance with a NaN or an infinite sample, as the reference's arithmetic gives it (`forward` returns a finite vector there:
            its ReLUs drop the NaNs).  The utterances lie side by side on one packed time axis per time resolution (ops.ragged_levels); the
            tables are built on the host from the lengths and uploaded once; nothing waits for the device.
            The 2-D convs run in exact f32 whatever `conv2d_precision` says (`last_conv2d_arithmetic` = "f32") unless
            `ragged_conv2d_precision` is "f16x3": the 36 block convs then run in split-f16 arithmetic (csrc/ragged2d16/, the segment form
            of the csrc/conv2d16/ kernel) with one overflow flag per utterance, read once after the call's last launch.  Unflagged
            utterances keep their rows; the flagged ones are extracted again as one ragged sub-batch in exact f32 and their rows
            scattered in, so that every row is what `forward` gives for that utterance alone under `conv2d_precision` = "f16x3", its own
            fallback included.  `last_split_fallback_rows` holds their sorted indices ([] without any), `split_fallbacks` rises by one for
            a call with any, and `last_conv2d_arithmetic` is "f16x3", "f16x3+f32" or, when every row fell back, "f32".  The attention's
            two 1x1 convs follow `precision`.
            Every utterance needs 1 280 samples (two pooled frames, `embed`'s rule); at most 1024 utterances and 32 * 80 * T_tot_0 * 4 <
            2^31 bytes per call (10 KB per frame for the largest tensor, several of which are live at once)."""
            if isinstance(wavs, tuple) and len(wavs) == 2 and isinstance(wavs[0], torch.Tensor) and wavs[0].dim() == 2:
                padded, lengths = wavs
                lengths = [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
                if len(lengths) != padded.shape[0] or (lengths and max(lengths) > padded.shape[1]):
                    raise _lib.SatError(f"extract_batch: {len(lengths)} lengths up to {max(lengths, default=0)} for a padded batch {tuple(padded.shape)}")
                tensors = [padded]
            else:
                tensors = list(wavs)
                if any(not isinstance(w, torch.Tensor) or w.dim() != 1 for w in tensors):
                    raise _lib.SatError("extract_batch: a list of 1-D tensors, or (padded [B, n_max], lengths)")
                lengths, padded = [int(w.shape[0]) for w in tensors], None
            if not lengths:
                raise _lib.SatError("extract_batch: an empty batch")
            if any(not w.is_cuda for w in tensors):
                raise _lib.SatError("x-vector extraction runs on the HIP device only (no CPU fallback)")
            if len(lengths) > ops.RAGGED_MAX_SEGMENTS:
                raise _lib.SatError(f"extract_batch: {len(lengths)} utterances in one call, at most {ops.RAGGED_MAX_SEGMENTS}")
            for i, n in enumerate(lengths):
                if pooled_frames(1 + n // ops.XV_HOP) < 2:
                    raise _lib.SatError(f"extract_batch: utterance {i} of {n} samples leaves {pooled_frames(1 + n // ops.XV_HOP)} pooled frame; the global "
                                        "context's unbiased deviation needs two (1 280 samples)")
            t_tot = ops.ragged_layout([1 + n // ops.XV_HOP for n in lengths])[2]
            if PLANES[0] * 80 * t_tot * 4 >= 2 ** 31:
                raise _lib.SatError(f"extract_batch: {t_tot} frames in one call, a 32-channel image of 2^31 bytes or more: split the batch")
            device = tensors[0].device
            W = self._prepare(device)
            if padded is None:
                padded = tensors[0].to(torch.float32).unsqueeze(0) if len(tensors) == 1 else \
                    torch.nn.utils.rnn.pad_sequence([w.to(torch.float32) for w in tensors], batch_first=True)
            padded = padded.to(torch.float32).contiguous()
            if not W["ragged16"]:
                self.last_split_fallback_rows = []
                return self._extract_packed(W, padded, lengths, None)
            # one zeroed flag per utterance (the call's own allocation), read once after everything is launched
            flags = torch.zeros(len(lengths), dtype=torch.int32, device=device)
            rows = self._extract_packed(W, padded, lengths, flags)
            bad = torch.nonzero(flags).flatten().tolist()
            self.last_split_fallback_rows = bad
            if bad:
                # these utterances left the f16 range: exact f32 for them, as one ragged sub-batch of their own
                self.split_fallbacks += 1
                idx = torch.tensor(bad, dtype=torch.long, device=device)
                rows[idx] = self._extract_packed(W, padded.index_select(0, idx), [lengths[i] for i in bad], None)
                self.last_conv2d_arithmetic = "f32" if len(bad) == len(lengths) else "f16x3+f32"
            return rows

        def _extract_packed(self, W, padded, lengths, overflow):
            """padded [B, n_max] f32 on the device and the host's lengths -> [B, 256]: the tables, the front end and `embed_segments`"""
            levels = ops.RaggedLevels(padded.device, n_samples=lengths)
            if self._mel_ranges is None or self._mel_ranges[0] is not W:
                self._mel_ranges = (W, ops.mel_filter_ranges(W["fb"]))
            mel = ops.melspec_logmel_segments(padded, levels[0], W["window"], W["fb"], W["coef"], fb_range=self._mel_ranges[1])
            return self.embed_segments(ops.instnorm_segments(mel, levels[0], out=mel), levels, overflow)

        def forward(self, x, target=None, taps=None):
            if target is not None:
                raise _lib.SatError("the MI355X x-vector extractor is inference only (target must be None)")
            if not x.is_cuda:
                raise _lib.SatError("x-vector extraction runs on the HIP device only (no CPU fallback)")
            x = x.to(torch.float32)
            if x.dim() == 1:
                x = x.unsqueeze(0)
            xv = self.embed(self.features(x.contiguous()), taps)
            return (torch.tensor(float("nan")), None), xv

    return Net
