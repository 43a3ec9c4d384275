#!/usr/bin/env python3
"""Prints one SHA-256 per case of the raw output bytes of the 2-D conv kernels of the ResNet x-vector extractor and of row_mean_std, per call
and per segment of a packed time axis, in both arithmetics, on seeded inputs; the overflow flags of the split-f16 cases beside them.  Two
builds of the library compute the same bits iff their listings are equal line by line (on the same device):
    python tools/conv2d_digest.py > new.txt;  SATOOLS_AMD_LIB=/path/to/other/libsatools_hip.so python tools/conv2d_digest.py > other.txt
No digest is kept anywhere: the comparison is always between two builds.

Shapes: H = 5 (two row tiles of 4, the second partial); width 70 at stride 1 and 70 -> 35 at stride 2 (a full column tile and a partial one
at 64 and at 32 output columns per block); B = 2; the segment forms on three segments of 70, 1 and 33 columns with NaN in every gap column
of the input and a sentinel in every gap column of the output (the whole buffer is hashed: an unwritten gap is part of the digest); without
an epilogue and with affine + ReLU.  The nine (Cin, Cout, ksize, stride) reach the stem and every instantiation of both arithmetics: f32
has 32 output channels per block (MT = 1) at Cout = 32 only, so (3 | 1) x (stride 1 | 2) each come at Cout = 32 and at Cout = 64; f16x3
has MT = 1 at Cout = 32 or stride 2, and its columns per block follow the stride."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"
H, W, B = 5, 70, 2
WIDTHS = (70, 1, 33)
CONVS = ((32, 32, 3, 1), (32, 64, 3, 2), (32, 64, 1, 2), (64, 64, 3, 1), (64, 64, 1, 1), (1, 32, 3, 1),
         (32, 32, 1, 1), (32, 32, 1, 2), (32, 32, 3, 2))
STD_T = (2, 65, 129)
SENTINEL = -7.0


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def rand(seed, *shape):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def table(ops, widths):
    off, length, t_tot = ops.ragged_layout(widths)
    return ops.RaggedLevel(off, length, t_tot, device=DEV)


def packed(ops, tab, seed, *lead):
    """segments of seeded values side by side, NaN in every gap column"""
    x = torch.full((*lead, tab.T_tot), float("nan"), device=DEV)
    for i, (o, n) in enumerate(zip(tab.host_off, tab.host_len)):
        x[..., o:o + n] = rand(seed + i, *lead, int(n))
    return x


def main():
    import satools_amd  # noqa: F401
    from satools_amd import _lib, ops
    print(f"# library {os.path.relpath(_lib.library_path(), ROOT) if _lib.library_path().startswith(ROOT) else 'SATOOLS_AMD_LIB'}  device {torch.cuda.get_device_name(0)}")
    tin = table(ops, WIDTHS)
    for n, (cin, cout, k, s) in enumerate(CONVS):
        w = rand(100 + n, cout, cin, k, k) * (2.0 / (cin * k * k) ** 0.5)
        wp = ops.pack_conv2d_weight(w)
        w16, d = ops.pack_conv2d_weight_f16x3(w) if cin != 1 else (None, None)
        x = rand(200 + n, B, cin, H, W)
        tout = table(ops, [(t - 1) // s + 1 for t in WIDTHS])
        xs = packed(ops, tin, 300 + 10 * n, 1, cin, H)
        ho = (H - 1) // s + 1
        for epi in ("none", "affine_relu"):
            sc, sh = (rand(400 + n, cout) + 1.5, rand(500 + n, cout)) if epi != "none" else (None, None)
            name = f"cin{cin}_cout{cout}_k{k}_s{s}_{epi}"
            out = lambda: torch.full((1, cout, ho, tout.T_tot), SENTINEL, device=DEV)
            print(f"conv2d                {name}  {digest(ops.conv2d(x, wp, k, s, sc, sh, relu=epi != 'none'))}")
            print(f"conv2d_segments       {name}  {digest(ops.conv2d_segments(xs, wp, k, s, tin, tout, sc, sh, relu=epi != 'none', out=out()))}")
            if cin == 1:
                continue
            flag, flags = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(len(WIDTHS), dtype=torch.int32, device=DEV)
            y = ops.conv2d_f16x3(x, w16, d, k, s, sc, sh, relu=epi != "none", overflow=flag)
            print(f"conv2d_f16x3          {name}  {digest(y)}  flag {flag.tolist()}")
            y = ops.conv2d_f16x3_segments(xs, w16, d, k, s, tin, tout, sc, sh, relu=epi != "none", overflow=flags, out=out())
            print(f"conv2d_f16x3_segments {name}  {digest(y)}  flags {flags.tolist()}")
    # a value at the split limit in segment 1 only: its flag alone, and the other segments' bits
    cin, cout, k, s = CONVS[0]
    w16, d = ops.pack_conv2d_weight_f16x3(rand(100, cout, cin, k, k) * (2.0 / (cin * k * k) ** 0.5))
    xs = packed(ops, tin, 300, 1, cin, H)
    xs[0, 3, 2, int(tin.host_off[1])] = 65520.0
    flags = torch.zeros(len(WIDTHS), dtype=torch.int32, device=DEV)
    y = ops.conv2d_f16x3_segments(xs, w16, d, k, s, tin, tin, overflow=flags, out=torch.full((1, cout, H, tin.T_tot), SENTINEL, device=DEV))
    keep = torch.cat([tin.segment(y, i).reshape(-1) for i in (0, 2)])            # segment 1's own outputs are unspecified
    print(f"conv2d_f16x3_segments 65520_in_segment_1  {digest(keep)}  flags {flags.tolist()}")
    x1 = tin.segment(xs, 1).reshape(1, cin, H, 1).contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.conv2d_f16x3(x1, w16, d, k, s, overflow=flag)
    print(f"conv2d_f16x3          65520_alone  flag {flag.tolist()}")
    for t in STD_T:
        print(f"row_mean_std          T{t}  {digest(ops.row_mean_std(rand(600 + t, B, 5, t)))}")
    tab = table(ops, STD_T)
    print(f"row_mean_std_segments T{'_'.join(map(str, STD_T))}  {digest(ops.row_mean_std_segments(packed(ops, tab, 700, 1, 5), tab))}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
