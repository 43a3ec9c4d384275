#!/usr/bin/env python3
"""Times x-vector extraction with the ResNet extractor (satools_amd.xvector_resnet) of utterances of UNEQUAL length: the per-utterance loop
`net(wav_i)` — what asv_eval.test_metrics does at batch_size 1 — against `net.extract_batch` (csrc/ragged2d/) at 8 and 32 utterances per call,
the latter in both arithmetics of the block convs: exact f32 and `ragged_conv2d_precision = "f16x3"` (csrc/ragged2d16/), a second net object
with the same weights so that neither side repacks anything inside a window.

Workload: 256 synthetic utterances whose lengths are drawn once, seeded, uniformly from 2 to 12 s (the workload of
tools/bench_xvector_ragged.py); every side extracts all 256 in the same order, in groups of consecutive utterances as test_metrics forms
them.  All sides run interleaved in every window; a window is one pass over the 256 utterances between two device synchronisations; the
median of `--windows` windows and their spread (min .. max) are reported per utterance, after `--warmup` untimed passes of each side.

The driver starts every step as a child process of its own under a time limit and stops at the first that fails:
    ragged      the loop against the two batch sizes in f32 and in f16x3, all five sides in the same windows; the largest x-vector
                difference between the two arithmetics, the f16x3 net's `split_fallbacks`, and per batch size whether the two medians differ
                by more than the windows' min .. max spread (only then is one side "faster"); also the host time of building and
                uploading the tables of one batch
    equal       one batch of 32 x 5 s through `forward` (the equal-length batch) against `extract_batch((padded, lengths))` in the same
                windows: what the packed layout costs or saves when nothing is ragged, beside the spread of `forward`'s own windows
    python tools/bench_xvector_resnet_ragged.py [--out profiles/xvector_resnet_ragged_bench.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"
N_UTT, SEED, BATCHES = 256, 20, (8, 32)
STEP_TIMEOUT = {"ragged": 420, "equal": 240}


def make_net(ragged="f32"):
    import satools_amd  # noqa: F401
    from satools_amd import synthetic, xvector_resnet
    net = xvector_resnet.build()(num_speakers=10)
    net.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True)
    net = net.to(DEV)
    net.conv2d_precision, net.ragged_conv2d_precision = "f32", ragged
    return net


def setup():
    import numpy as np
    import torch
    net = make_net()
    lengths = np.random.default_rng(SEED).integers(2 * 16000, 12 * 16000 + 1, N_UTT).tolist()
    pool = (torch.rand(sum(lengths), generator=torch.Generator().manual_seed(SEED)) - 0.5).to(DEV)
    wavs, pos = [], 0
    for n in lengths:
        wavs.append(pool[pos:pos + n])
        pos += n
    return net, wavs, lengths


def groups(n):
    return [list(range(i, min(i + n, N_UTT))) for i in range(0, N_UTT, n)]


def window(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v, per=1):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4), "max_ms": round(max(v) / per, 4)}


def step_ragged(a):
    import torch
    from satools_amd import ops
    net, wavs, lengths = setup()
    net16 = make_net("f16x3")
    with torch.no_grad():
        sides = {"loop": lambda: [net(w)[1] for w in wavs]}
        for n in BATCHES:
            sides[f"batch{n}"] = (lambda n: lambda: [net.extract_batch([wavs[i] for i in g]) for g in groups(n)])(n)
            sides[f"batch{n}_f16x3"] = (lambda n: lambda: [net16.extract_batch([wavs[i] for i in g]) for g in groups(n)])(n)
        ref = torch.cat(sides["loop"]())
        rows = {k: torch.cat(fn()) for k, fn in sides.items() if k != "loop"}
        diffs = {k: float((v - ref).abs().max()) for k, v in rows.items()}
        diffs16 = {f"batch{n}": float((rows[f"batch{n}_f16x3"] - rows[f"batch{n}"]).abs().max()) for n in BATCHES}
        for fn in sides.values():
            for _ in range(a.warmup):
                fn()
        times = {k: [] for k in sides}
        for _ in range(a.windows):
            for k, fn in sides.items():
                times[k].append(window(fn))
    rec = {"measurement": "xvector_resnet_ragged_extraction", "utterances": N_UTT, "seconds": [2, 12], "seed": SEED,
           "frames_total": sum(1 + n // 160 for n in lengths), "windows": a.windows, "unit": "ms per utterance", "max_abs_diff_vs_loop": diffs,
           "max_abs_diff_f16x3_vs_f32": diffs16}
    for k, v in times.items():
        rec[k] = stats(v, N_UTT)
        if k != "loop":
            rec["ratio_loop_over_" + k] = round(statistics.median(times["loop"]) / statistics.median(v), 3)
            rec[k + "_faster_than_loop_in_every_window"] = all(b < l for b, l in zip(v, times["loop"]))
    for n in BATCHES:
        a32, a16 = times[f"batch{n}"], times[f"batch{n}_f16x3"]
        gap = (statistics.median(a32) - statistics.median(a16)) / N_UTT
        spread = max(max(a32) - min(a32), max(a16) - min(a16)) / N_UTT
        rec[f"ratio_batch{n}_f32_over_f16x3"] = round(statistics.median(a32) / statistics.median(a16), 3)
        rec[f"batch{n}_f32_minus_f16x3_ms"] = round(gap, 4)
        rec[f"batch{n}_windows_spread_ms"] = round(spread, 4)
        # "faster" is claimed only if the medians differ by more than the windows' min .. max spread
        rec[f"batch{n}_verdict"] = "f16x3 faster" if gap > spread else ("f32 faster" if -gap > spread else "no difference beyond the spread")
    rec["split_fallbacks_f16x3"], rec["last_conv2d_arithmetic_f16x3"] = net16.split_fallbacks, net16.last_conv2d_arithmetic
    # host time of one batch's tables (the four layouts, the column index, the copy into the page-locked block and the asynchronous
    # upload), no device wait
    for n in BATCHES:
        g = groups(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            for idx in g:
                ops.RaggedLevels(torch.device(DEV), n_samples=[lengths[i] for i in idx])
        rec[f"table_host_us_per_batch{n}"] = round((time.perf_counter() - t0) / (5 * len(g)) * 1e6, 1)
        torch.cuda.synchronize()
    print(json.dumps(rec), flush=True)


def step_equal(a):
    import torch
    from satools_amd import synthetic
    net, _, _ = setup()
    wav = (synthetic.rand_batch(1, 32, 80000) - 0.5).to(DEV)
    with torch.no_grad():
        sides = {"forward_batch32": lambda: net(wav)[1], "extract_batch32_padded_argument": lambda: net.extract_batch((wav, [80000] * 32))}
        diff = float((sides["forward_batch32"]() - sides["extract_batch32_padded_argument"]()).abs().max())
        for fn in sides.values():
            for _ in range(a.warmup):
                fn()
        times = {k: [] for k in sides}
        for _ in range(a.windows):
            for k, fn in sides.items():
                times[k].append(statistics.mean(window(fn) for _ in range(a.iters)))
    rec = {"measurement": "xvector_resnet_ragged_equal_lengths_32x5s", "windows": a.windows, "iters_per_window": a.iters, "unit": "ms per batch",
           "max_abs_diff_extract_vs_forward": diff}
    for k, v in times.items():
        rec[k] = stats(v)
    f, e = rec["forward_batch32"], rec["extract_batch32_padded_argument"]
    rec["forward_spread_ms"] = round(f["max_ms"] - f["min_ms"], 4)
    rec["extract_minus_forward_ms"] = round(e["median_ms"] - f["median_ms"], 4)
    rec["ratio_forward_over_extract"] = round(f["median_ms"] / e["median_ms"], 3)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default="ragged,equal")
    ap.add_argument("--step", default=None, choices=("ragged", "equal"))
    a = ap.parse_args()
    if a.step:
        return {"ragged": step_ragged, "equal": step_equal}[a.step](a)
    lines = []
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--warmup", str(a.warmup),
               "--windows", str(a.windows), "--iters", str(a.iters)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
        if a.out:
            with open(a.out, "w") as f:
                f.write("".join(l + "\n" for l in lines))
        if p.returncode != 0:
            sys.stderr.write(f"step {step} ended with status {p.returncode}: nothing further is started\n")
            raise SystemExit(p.returncode if p.returncode > 0 else 1)


if __name__ == "__main__":
    main()
