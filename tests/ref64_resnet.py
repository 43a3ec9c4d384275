"""Float64 restatements of the ResNet x-vector extractor (egs/asv/voxceleb/local/tuning/resnet.py; sidekit/archi.py PreHalfResNet34,
sidekit/nn.py SELayer / ResNetBasicBlock, sidekit/pooling.py MeanStdPooling / AttentivePooling), written from the reference's formulas
in float64 torch on the CPU, as tests/ref64.py does for the ECAPA net's small operations: a function whose result involves a reduction
also returns, in a dict, the sums of absolute terms a rounding-error bound needs.  Inputs are float32 tensors (or anything
torch.as_tensor takes).  `ref64.in_float32()` switches these functions to float32 too.  A plain module: no fixtures, no GPU.
tests/test_ref64_resnet.py pins `forward` against the reference's own outputs.

LAYOUT: images are [B, C, H, W] and nothing here cares which axis is time; `forward` runs the reference's own [B, 1, T, 80]."""
import torch
import torch.nn.functional as F

import ref64
from ref64 import U  # noqa: F401

BLOCKS = (3, 4, 6, 3)
BN_EPS = 1e-5


def _d(x):
    return ref64._d(x)


def conv2d(x, w, stride=1, scale=None, shift=None, relu=False):
    """Conv2d(bias=False, padding = ksize // 2) -> * scale[co] + shift[co] (after the sum) -> optional ReLU.
    x [B, Cin, H, W], w [Cout, Cin, k, k].  aux: "sum" = the plain conv, S = sum |w x| per output, "affine" = the value before the ReLU"""
    x, w = _d(x), _d(w)
    pad = w.shape[2] // 2
    s = F.conv2d(x, w, None, stride=stride, padding=pad)
    S = F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=pad)
    v = s
    if scale is not None:
        v = s * _d(scale).view(1, -1, 1, 1) + _d(shift).view(1, -1, 1, 1)
    return (torch.relu(v) if relu else v), {"sum": s, "S": S, "affine": v}


def batchnorm_affine(weight, bias, mean, var, eps=BN_EPS):
    """BatchNorm in eval as y = x * scale + shift"""
    scale = _d(weight) / torch.sqrt(_d(var) + eps)
    return scale, _d(bias) - _d(mean) * scale


def se_scale_add_relu(z, gate_logits, r):
    """relu(z * sigmoid(g[b][c]) + r), z / r [B, C, ...], g [B, C].  aux: "gate", "prod" = |z gate|, "pre" = the value before the ReLU"""
    z, r = _d(z), _d(r)
    g = _d(gate_logits).reshape(z.shape[0], z.shape[1], *([1] * (z.dim() - 2)))
    gate = torch.sigmoid(g)
    v = z * gate
    pre = v + r
    return torch.relu(pre), {"gate": gate, "prod": v.abs(), "pre": pre}


def se_gate_logits(z, fc0, fc2):
    """SELayer up to its Sigmoid: mean over H x W -> Linear (no bias) -> ReLU -> Linear (no bias); z [B, C, H, W] -> [B, C]"""
    z = _d(z)
    m = z.flatten(2).sum(2) / (z.shape[2] * z.shape[3])
    return torch.relu(m @ _d(fc0).t()) @ _d(fc2).t()


def mean_std(x):
    """rows along the last axis: mean and UNBIASED standard deviation (torch.std), NaN for one value.
    aux: S1 = sum |x|, S2 = sum (x - mean)^2"""
    x = _d(x)
    T = x.shape[-1]
    mean = x.sum(-1) / T
    d = x - mean.unsqueeze(-1)
    S2 = (d * d).sum(-1)
    std = torch.sqrt(S2 / (T - 1)) if T > 1 else torch.full_like(mean, float("nan"))
    return mean, std, {"S1": x.abs().sum(-1), "S2": S2}


def attention_hidden(x, w0, b0, bn_scale, bn_shift):
    """AttentivePooling's first half with global context: the frames [B, D, T] concatenated with their mean and unbiased deviation over
    time (repeated at every frame) -> 1x1 conv [A, 3 D] + bias -> ReLU -> BatchNorm(eval) -> Tanh.  Returns a [B, A, T].
    aux: S = sum |w| |input| of the conv per output, "lin" = the conv's output, "gc" [B, 2 D]"""
    x, w0 = _d(x), _d(w0).reshape(_d(w0).shape[0], -1)
    mean, std, _ = mean_std(x)
    gc = torch.cat([mean, std], dim=1)
    full = torch.cat([x, gc.unsqueeze(2).expand(-1, -1, x.shape[2])], dim=1)          # [B, 3 D, T]
    lin = torch.einsum("ak,bkt->bat", w0, full) + _d(b0).view(1, -1, 1)
    S = torch.einsum("ak,bkt->bat", w0.abs(), full.abs()) + _d(b0).abs().view(1, -1, 1)
    a = torch.tanh(torch.relu(lin) * _d(bn_scale).view(1, -1, 1) + _d(bn_shift).view(1, -1, 1))
    return a, {"S": S, "lin": lin, "gc": gc}


def attentive_pooling_gc(x, w0, b0, bn_scale, bn_shift, w4, b4):
    """AttentivePooling(global_context=True).forward on [B, D, T] -> [B, 2 D]: weighted means, then weighted deviations
    sqrt(max(sum w x^2 - mu^2, 1e-9)).  aux: "lin" (the first conv's output), "a", "logits", S_hidden / S_logits = sum |w| |input| of the
    two convs, and ref64.attentive_stats's sums"""
    a, aux1 = attention_hidden(x, w0, b0, bn_scale, bn_shift)
    w4 = _d(w4).reshape(_d(w4).shape[0], -1)
    logits = torch.einsum("da,bat->bdt", w4, a) + _d(b4).view(1, -1, 1)
    S_logits = torch.einsum("da,bat->bdt", w4.abs(), a.abs()) + _d(b4).abs().view(1, -1, 1)
    mean, std, aux = ref64.attentive_stats(x, logits)
    return torch.cat([mean, std], dim=1), dict(aux, lin=aux1["lin"], a=a, logits=logits, S_hidden=aux1["S"], S_logits=S_logits)


def forward(sd, feats):
    """the whole Net from the front end's output to the x-vector: sd = the reference's state dict, feats [B, 80, T] (log-mel after
    InstanceNorm).  Returns (x_vector [B, 256], taps): "bn1" and "layer1" .. "layer4" in the reference's [B, C, T, F] layout, "pooled"
    [B, 5120]"""
    def bn(prefix):
        return batchnorm_affine(sd[prefix + ".weight"], sd[prefix + ".bias"], sd[prefix + ".running_mean"], sd[prefix + ".running_var"])

    taps = {}
    x = _d(feats).unsqueeze(1).permute(0, 1, 3, 2)                                       # [B, 1, T, 80]
    p = "sequence_network."
    x = conv2d(x, sd[p + "conv1.weight"], 1, *bn(p + "bn1"), relu=True)[0]
    taps["bn1"] = x
    for li, n in enumerate(BLOCKS):
        for j in range(n):
            q = f"{p}layer{li + 1}.{j}."
            stride = 2 if (li > 0 and j == 0) else 1
            out = conv2d(x, sd[q + "conv1.weight"], stride, *bn(q + "bn1"), relu=True)[0]
            out = conv2d(out, sd[q + "conv2.weight"], 1, *bn(q + "bn2"))[0]
            g = se_gate_logits(out, sd[q + "se.fc.0.weight"], sd[q + "se.fc.2.weight"])
            r = conv2d(x, sd[q + "shortcut.0.weight"], stride, *bn(q + "shortcut.1"))[0] if (q + "shortcut.0.weight") in sd else x
            x = se_scale_add_relu(out, g, r)[0]
        taps[f"layer{li + 1}"] = x
    x = x.permute(0, 1, 3, 2).flatten(1, 2)                                              # [B, C * F, T']
    a = "stat_pooling.attention."
    pooled = attentive_pooling_gc(x, sd[a + "0.weight"], sd[a + "0.bias"], *bn(a + "2"), sd[a + "4.weight"], sd[a + "4.bias"])[0]
    taps["pooled"] = pooled
    sc, sh = bn("before_speaker_embedding.bn_be")
    e = (pooled @ _d(sd["before_speaker_embedding.lin_be.weight"]).t()) * sc + sh
    return ref64.l2norm(e)[0], taps
