#!/usr/bin/env python3
"""Times the forward of the ResNet x-vector extractor (satools_amd.xvector_resnet) against the same architecture in plain torch.nn
modules on the same device with the same weights, `channels_last` as the reference runs it (sidekit/archi.py:12-15), for
a batch of 32 utterances of 5 s and for one utterance of 5 s.  Both sides start from the same front-end features (the front end is the
ECAPA net's and is timed with the HIP side only as part of `hip_with_front_end`).

A third side is the same HIP net with `conv2d_precision = "f16x3"` (the blocks' 2-D convs in split-f16 arithmetic, csrc/conv2d16/): the
comparison that matters for it is `hip_f16x3` against `hip` (exact f32) in the same windows.

All sides run interleaved in every window; a window is `--iters` forwards between two device synchronisations; the median of
`--windows` windows and their spread (min .. max) are reported, after `--warmup` untimed forwards of each side.

The driver starts every step as a child process of its own under a time limit and stops at the first that fails:
    batch32, single          the two timings, one JSON line each
    kernels                  the per-kernel split of three batch-32 forwards with the f16x3 convs: `rocprofv3 --kernel-trace --stats` around
                             the `once` step, the ten kernels with the largest total time as one JSON line
    python tools/bench_xvector_resnet.py [--out profiles/xvector_resnet_f16x3_bench.jsonl]

Arithmetic floor: 36 + 1 convs are 22.9 GFLOP per 5 s utterance, 0.73 TFLOP per batch of 32: 4.7 ms at the 155 TFLOP/s the f32 MFMA
measures on this device."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"
STEP_TIMEOUT = {"batch32": 420, "single": 240, "kernels": 300}


def torch_twin(sd):
    """the reference's architecture from plain torch.nn modules (time innermost is NOT used here: [B, 1, T, 80] as the reference)"""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class Block(nn.Module):
        def __init__(self, cin, cout, stride, shortcut):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False), nn.BatchNorm2d(cout)
            self.conv2, self.bn2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout)
            self.se = nn.Module()
            self.se.fc = nn.Sequential(nn.Linear(cout, cout // 16, bias=False), nn.ReLU(), nn.Linear(cout // 16, cout, bias=False), nn.Sigmoid())
            self.shortcut = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout)) if shortcut else nn.Sequential()

        def forward(self, x):
            out = F.relu(self.bn1(self.conv1(x)))
            out = self.bn2(self.conv2(out))
            out = out * self.se.fc(out.mean((2, 3))).view(out.shape[0], -1, 1, 1)
            return F.relu(out + self.shortcut(x))

    class Twin(nn.Module):
        def __init__(self):
            super().__init__()
            sn = nn.Module()
            sn.conv1, sn.bn1 = nn.Conv2d(1, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32)
            cin = 32
            for i, (c, n) in enumerate(zip((32, 64, 128, 256), (3, 4, 6, 3))):
                blocks = []
                for j in range(n):
                    blocks.append(Block(cin, c, 2 if (i and j == 0) else 1, j == 0))
                    cin = c
                setattr(sn, f"layer{i + 1}", nn.Sequential(*blocks))
            self.sequence_network = sn
            sp = nn.Module()
            sp.attention = nn.Sequential(nn.Conv1d(7680, 128, 1), nn.ReLU(), nn.BatchNorm1d(128), nn.Tanh(), nn.Conv1d(128, 2560, 1), nn.Softmax(dim=2))
            self.stat_pooling = sp
            be = nn.Sequential()
            be.add_module("lin_be", nn.Linear(5120, 256, bias=False))
            be.add_module("bn_be", nn.BatchNorm1d(256))
            self.before_speaker_embedding = be

        def forward(self, feats):
            sn = self.sequence_network
            x = feats.unsqueeze(1).permute(0, 1, 3, 2).contiguous(memory_format=torch.channels_last)
            x = F.relu(sn.bn1(sn.conv1(x)))
            x = sn.layer4(sn.layer3(sn.layer2(sn.layer1(x))))
            x = x.permute(0, 1, 3, 2).flatten(1, 2)
            gc = torch.cat([x.mean(2), x.std(2)], 1)
            w = self.stat_pooling.attention(torch.cat([x, gc.unsqueeze(2).repeat(1, 1, x.shape[-1])], 1))
            mu = (x * w).sum(2)
            rh = torch.sqrt(((x ** 2 * w).sum(2) - mu ** 2).clamp(min=1e-9))
            return F.normalize(self.before_speaker_embedding(torch.cat((mu, rh), 1)), dim=1)

    twin = Twin()
    missing = twin.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("preprocessor.", "after_speaker_embedding."))}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return twin.eval().to(DEV).to(memory_format=torch.channels_last)


def setup(B):
    import torch
    import satools_amd  # noqa: F401
    from satools_amd import synthetic, xvector_resnet
    torch.backends.cudnn.benchmark = True              # MIOpen picks its fastest conv per shape during the warm-up
    sd = synthetic.xvector_resnet_state(0, 10)
    net = xvector_resnet.build()(num_speakers=10)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    net.conv2d_precision = "f32"
    net16 = xvector_resnet.build()(num_speakers=10)
    net16.load_state_dict(sd, strict=True)
    net16 = net16.to(DEV)
    net16.conv2d_precision = "f16x3"
    wav = synthetic.rand_batch(1, B, 80000).to(DEV) - 0.5
    feats = net.features(wav)
    return net, net16, torch_twin(sd), wav, feats


def window(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def step_time(name, B, a):
    import torch
    net, net16, twin, wav, feats = setup(B)
    with torch.no_grad():
        sides = {"hip": lambda: net.embed(feats), "hip_f16x3": lambda: net16.embed(feats), "torch_channels_last": lambda: twin(feats),
                 "hip_with_front_end": lambda: net(wav)[1]}
        x0, x1, x2 = sides["hip"](), sides["torch_channels_last"](), sides["hip_f16x3"]()
        for fn in sides.values():
            for _ in range(a.warmup):
                fn()
        times = {k: [] for k in sides}
        for _ in range(a.windows):
            for k, fn in sides.items():
                times[k].append(window(fn, a.iters))
    rec = {"measurement": f"xvector_resnet_forward_{name}", "shape": {"B": B, "samples": 80000, "frames": int(feats.shape[2])},
           "windows": a.windows, "iters_per_window": a.iters, "max_abs_diff_xvector": float((x0 - x1).abs().max()),
           "max_abs_diff_xvector_f16x3_vs_f32": float((x2 - x0).abs().max()), "f16x3_arithmetic_ran": net16.last_conv2d_arithmetic,
           "f16x3_split_fallbacks": int(net16.split_fallbacks)}
    for k, v in times.items():
        rec[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    rec["ratio_torch_over_hip"] = round(rec["torch_channels_last"]["median_ms"] / rec["hip"]["median_ms"], 3)
    rec["ratio_f32_over_f16x3"] = round(rec["hip"]["median_ms"] / rec["hip_f16x3"]["median_ms"], 3)
    rec["f16x3_mfma_floor_ms"] = round(3 * 22.9e9 * B / 2.5e15 * 1e3, 3)          # three products per term at the f16 peak
    rec["conv_gflop"] = round(22.9 * B, 1)
    rec["f32_mfma_floor_ms"] = round(22.9e9 * B / 155e12 * 1e3, 3)
    print(json.dumps(rec), flush=True)


def step_once(a):
    import torch
    _, net16, _, _, feats = setup(32)
    with torch.no_grad():
        for _ in range(3):
            net16.embed(feats)
        torch.cuda.synchronize()


def step_kernels(a):
    """one process under rocprofv3 (the program goes after `--`), its kernel statistics summed by kernel name"""
    d = tempfile.mkdtemp(prefix="xvr_prof_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                        "--step", "once"], check=True, timeout=STEP_TIMEOUT["kernels"] - 20, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(files[0])))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:10]
        rec = {"measurement": "xvector_resnet_f16x3_kernel_split_batch32", "forwards_traced": 3, "setup_included": True,
               "kernels": [{"name": r["Name"][:70], "calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                            "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in top]}
        print(json.dumps(rec), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=("batch32", "single", "once", "kernels"))
    a = ap.parse_args()
    if a.step == "batch32":
        return step_time("batch32_5s", 32, a)
    if a.step == "single":
        return step_time("single_5s", 1, a)
    if a.step == "once":
        return step_once(a)
    if a.step == "kernels":
        return step_kernels(a)
    lines = []
    for step in ("batch32", "single", "kernels"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--warmup", str(a.warmup),
               "--windows", str(a.windows), "--iters", str(a.iters)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(f"step {step} ended with status {p.returncode}: nothing further is started\n")
            raise SystemExit(p.returncode if p.returncode > 0 else 1)
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(l + "\n" for l in lines))


if __name__ == "__main__":
    main()
