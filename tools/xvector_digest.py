#!/usr/bin/env python3
"""Prints one SHA-256 per case of the raw output bytes of the ECAPA x-vector extractor's kernels that exist in a row form (csrc/xvector.hip)
and a segment form (csrc/ragged/xvector_ragged.hip) — the log-mel front end, InstanceNorm, the row mean, the SE gate, the attentive statistics
and the Res2 chain — and of the nets built on them, on seeded inputs.  Two builds of the library compute the same bits iff their listings
are equal line by line (on the same device):
    python tools/xvector_digest.py > new.txt;  SATOOLS_AMD_LIB=/path/to/other/libsatools_hip.so python tools/xvector_digest.py > other.txt
No digest is kept anywhere: the comparison is always between two builds.

Shapes: the reductions at C = 5 and 8 (a block of four waves ends inside a row of segments; the gate kernel's group of 8 channels is met and
straddled) on lengths 4, 63, 64, 65, 129 (below, at and above one and two strides of the 64 lanes); the front end at 513 samples (the
shortest), 640 (a fifth frame: a second block of four), 10079 / 10080 / 10240 (63, 64, 65 frames), each in a call of its own and all in one
ragged batch; the segment chain on lengths 7 (< the halo), 64, 65, 129, 193 with both centres forced, for (pieces, dilation) = (7, 2),
(7, 4), (3, 1); the per-call chain in its narrow instantiation (B = 2, T = 129, 7 pieces) and its wide one (B = 128, T = 129, 3 pieces:
B * ceil(T / 128) = 256).  Every segment case has NaN in the gap columns of its inputs and a sentinel in its output buffer, and the whole
buffer is hashed: an unwritten gap is part of the digest, a written one changes it."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"
CHANNELS = (5, 8)
LENGTHS = (4, 63, 64, 65, 129)
SAMPLES = (513, 640, 10079, 10080, 10240)
CHAIN_LENGTHS = (7, 64, 65, 129, 193)
CHAIN_CASES = ((7, 2), (7, 4), (3, 1))                      # (pieces, dilation)
CHAIN_CALLS = (("narrow", 2, 129, 7, 2), ("wide", 128, 129, 3, 1))   # B, T, pieces, dilation
NET_SAMPLES = (8000, 10079, 24123)
SENTINEL = -7.0


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def packed(tab, segments):
    """per-utterance CPU tensors [C, T_i] side by side on the table's axis, NaN in every gap column -> [1, C, T_tot] on the device"""
    x = torch.full((segments[0].shape[0], tab.T_tot), float("nan"))
    for s, o, n in zip(segments, tab.host_off, tab.host_len):
        x[:, int(o):int(o) + int(n)] = s
    return x.to(DEV).unsqueeze(0)


def sentinel(*shape):
    return torch.full(shape, SENTINEL, device=DEV)


def reductions(ops):
    tab = ops.RaggedTable(torch.device(DEV), frames=LENGTHS)
    for C in CHANNELS:
        xs = [randn(1000 + 10 * C + i, C, t) * (0.5 + i) + (i - 2.0) for i, t in enumerate(LENGTHS)]
        ls = [randn(2000 + 10 * C + i, C, t) for i, t in enumerate(LENGTHS)]
        sk = [[randn(3000 + 100 * k + 10 * C + i, C, t) for i, t in enumerate(LENGTHS)] for k in range(3)]
        g = randn(4000 + C, len(LENGTHS), C).to(DEV)
        for i, t in enumerate(LENGTHS):
            x, lg = torch.stack([xs[i], -xs[i]]).to(DEV), torch.stack([ls[i], 2 * ls[i]]).to(DEV)           # B = 2
            name = f"C{C}_T{t}"
            print(f"instnorm_rows             {name}  {digest(ops.instnorm_rows(x))}")
            print(f"row_mean                  {name}  {digest(ops.row_mean(x))}")
            print(f"attentive_stats           {name}  {digest(ops.attentive_stats(x, lg))}")
            for n in range(4):
                skips = [torch.stack([s[i], s[i] + 1]).to(DEV) for s in sk[:n]]
                print(f"se_gate_add               {name}_skips{n}  {digest(ops.se_gate_add(x, torch.stack([g[i], -g[i]]), skips))}")
        name = f"C{C}_T{'_'.join(map(str, LENGTHS))}"
        x, lg = packed(tab, xs), packed(tab, ls)
        print(f"instnorm_segments         {name}  {digest(ops.instnorm_segments(x, tab, out=sentinel(1, C, tab.T_tot)))}")
        print(f"row_mean_segments         {name}  {digest(ops.row_mean_segments(x, tab))}")
        print(f"attentive_stats_segments  {name}  {digest(ops.attentive_stats_segments(x, lg, tab))}")
        for n in range(4):
            wide = sentinel(1, C + 3, tab.T_tot)                                                               # a channel slice of a wider tensor
            ops.se_gate_add_segments(x, g, [packed(tab, s) for s in sk[:n]], tab, out=wide[:, 2:2 + C])
            print(f"se_gate_add_segments      {name}_skips{n}  {digest(wide)}")


def front_end(ops):
    from satools_amd import xvector
    window, fb = torch.hann_window(400, periodic=True).to(DEV), xvector.mel_filterbank().t().contiguous().to(DEV)
    wavs = [randn(5000 + i, n) * 0.1 for i, n in enumerate(SAMPLES)]
    for w in wavs:
        print(f"melspec_logmel            n{w.shape[0]}  {digest(ops.melspec_logmel(torch.stack([w, w.flip(0)]).to(DEV), window, fb, 0.97))}")
    tab = ops.RaggedTable(torch.device(DEV), n_samples=SAMPLES)
    padded = torch.full((len(wavs), max(SAMPLES)), float("nan"))
    for i, w in enumerate(wavs):
        padded[i, :w.shape[0]] = w
    padded, out = padded.to(DEV), sentinel(1, fb.shape[0], tab.T_tot)
    lo, hi = ops.mel_filter_ranges(fb)
    # (ops.melspec_logmel_segments allocates its result: the entry point itself, on a buffer that holds the sentinel)
    ops.check(ops.lib().sat_melspec_logmel_segments_f32(ops.ptr(padded), ops.ptr(tab.n_samples), tab.n_samples_host, ops.ptr(tab.seg_off),
                                                        ops.ptr(tab.seg_len), ops.ptr(out), ops.ptr(window), ops.ptr(fb), ops.ptr(lo), ops.ptr(hi),
                                                        tab.B, padded.shape[1], tab.T_tot, fb.shape[0], 0.97, ops.stream()),
              "sat_melspec_logmel_segments_f32")
    print(f"melspec_logmel_segments   n{'_'.join(map(str, SAMPLES))}  {digest(out)}")


def chain_weights(seed, nums):
    w = randn(seed, nums, 3, 64, 64) * (64 * 3) ** -0.5
    return w.to(DEV), (torch.rand(nums, 64, generator=torch.Generator().manual_seed(seed + 1)) + 0.5).to(DEV), (randn(seed + 2, nums, 64) * 0.1).to(DEV)


def chains(ops):
    tab = ops.RaggedTable(torch.device(DEV), frames=CHAIN_LENGTHS)
    for k, (nums, dil) in enumerate(CHAIN_CASES):
        w, sc, sh = chain_weights(6000 + 10 * k, nums)
        C = (nums + 1) * 64
        y = packed(tab, [randn(6100 + 10 * k + i, C, t) for i, t in enumerate(CHAIN_LENGTHS)])
        for centre in (64, 128):
            z = ops.res2_chain_segments(y, w, sc, sh, dil, tab, centre=centre, out=sentinel(1, C, tab.T_tot))
            print(f"res2_chain_segments       pieces{nums}_dil{dil}_centre{centre}_T{'_'.join(map(str, CHAIN_LENGTHS))}  {digest(z)}")
    for k, (name, B, T, nums, dil) in enumerate(CHAIN_CALLS):
        w, sc, sh = chain_weights(7000 + 10 * k, nums)
        y = randn(7100 + k, B, (nums + 1) * 64, T).to(DEV)
        print(f"res2_chain                {name}_B{B}_T{T}_pieces{nums}_dil{dil}  {digest(ops.res2_chain(y, w, sc, sh, dil, out=torch.full_like(y, SENTINEL)))}")


def nets():
    from satools_amd import synthetic, xvector, xvector_resnet
    net = xvector.build()(num_speakers=10)
    net.load_state_dict(synthetic.xvector_state(0, 10), strict=True)
    net = net.to(DEV)
    wavs = [synthetic.harm_batch([20 + i], n)[0] for i, n in enumerate(NET_SAMPLES)]
    print(f"xvector forward           B1_n{NET_SAMPLES[0]}  {digest(net(wavs[0].to(DEV))[1])}")
    print(f"xvector forward           B2_n{NET_SAMPLES[0]}  {digest(net(torch.stack([wavs[0], wavs[0].flip(0)]).to(DEV))[1])}")
    print(f"xvector extract_batch     n{'_'.join(map(str, NET_SAMPLES))}  {digest(net.extract_batch([w.to(DEV) for w in wavs]))}")
    res = xvector_resnet.build()(num_speakers=10)
    res.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True)
    res = res.to(DEV)
    print(f"xvector_resnet forward    B1_n{NET_SAMPLES[1]}  {digest(res(wavs[1].to(DEV))[1])}")


def main():
    import satools_amd  # noqa: F401
    from satools_amd import _lib, ops
    print(f"# library {os.path.relpath(_lib.library_path(), ROOT) if _lib.library_path().startswith(ROOT) else 'SATOOLS_AMD_LIB'}  device {torch.cuda.get_device_name(0)}")
    reductions(ops)
    front_end(ops)
    chains(ops)
    nets()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
