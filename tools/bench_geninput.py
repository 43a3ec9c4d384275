#!/usr/bin/env python3
"""Times the fused generator-input launch (ops.generator_input, csrc/geninput/) against what it replaces: the `.contiguous()` copy of the
extractor's [B, T, C] bottleneck through its permuted view, sat_f0_stats_f32, sat_f0_apply_f32, the `.contiguous()` copy of the permuted
track, and sat_assemble_input_f32.  Both sides start from the same tensors (bn as the extractor leaves it, the raw track [1, B, T']) and
end with the generator's input; the fused side takes its statistics from sat_f0_stats_f32 too (the batch-coupled case), so the pair
differs by the launches alone.

Shapes: the benchmark's 32 x 250 frames x (256 + 1 + 247) and the 257-channel form (no speaker rows).
Sides alternate call by call inside every window; a timed call is the Python call and a device synchronisation.  After `--warmup` untimed
calls, the median of `--windows` windows and their spread (min .. max) are reported, and the two results are compared bit for bit.
Prints one JSON line per shape; --out FILE also writes them to a file.

    python tools/bench_geninput.py [--out profiles/geninput_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import satools_amd  # noqa: E402,F401
from satools_amd import _lib, ops  # noqa: E402

DEV = "cuda"
SHAPES = [(32, 256, 250, 251, 247), (32, 256, 250, 251, 0)]


def stats(ts):
    return {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geninput.py needs the GPU: a time taken elsewhere says nothing")
    recs = []
    for B, c_bn, T, t_f0, n_spk in SHAPES:
        g = torch.Generator().manual_seed(0)
        btc = torch.randn(B, T, c_bn, generator=g).to(DEV)
        f0 = 80.0 + 220.0 * torch.rand(1, B, t_f0, generator=g)
        f0 = torch.where(torch.rand(1, B, t_f0, generator=g) < 0.6, f0, torch.zeros_like(f0)).to(DEV)
        spk = torch.nn.functional.one_hot(torch.arange(B) % n_spk, n_spk).float().to(DEV) if n_spk else None
        out = {}

        def calls():
            bn = btc.permute(0, 2, 1).contiguous()
            f0_d = f0.clone()                                   # (the in-place normalisation: the fused side does not write its input)
            ops.f0_norm_transform_(f0_d)
            f0_b = f0_d.permute(1, 0, 2).contiguous()
            if spk is None:
                x = torch.empty(B, c_bn + 1, T, dtype=torch.float32, device=DEV)
                _lib.check(_lib.lib().sat_assemble_input_f32(_lib.ptr(bn), _lib.ptr(f0_b), None, _lib.ptr(x), B, c_bn, T, t_f0, 0, _lib.stream()),
                           "sat_assemble_input_f32")
                out["calls"] = x
            else:
                out["calls"] = ops.assemble_input(bn, f0_b.reshape(B, -1), spk, n_spk)

        def fused():
            st = torch.empty(1, 2, dtype=torch.float32, device=DEV)
            _lib.check(_lib.lib().sat_f0_stats_f32(_lib.ptr(f0), f0.numel(), _lib.ptr(st), _lib.stream()), "sat_f0_stats_f32")
            out["fused"], out["norm"] = ops.generator_input(btc.permute(0, 2, 1), f0, st, None, 0, None, spk)

        sides = [("calls", calls), ("fused", fused)]
        for _ in range(a.warmup):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in sides}
        for _ in range(a.windows):
            spent = {name: 0.0 for name, _ in sides}
            for _ in range(a.calls):                            # alternated call by call: both sides see the same clocks
                for name, fn in sides:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    spent[name] += time.perf_counter() - t0
            for name in spent:
                times[name].append(1e6 * spent[name] / a.calls)
        rec = {"measurement": "geninput", "shape": {"B": B, "C_bn": c_bn, "T": T, "T_f0": t_f0, "n_spk": n_spk}, "windows": a.windows,
               "calls_per_window": a.calls, "calls": stats(times["calls"]), "fused": stats(times["fused"]),
               "equal_bits": bool(torch.equal(out["calls"].view(torch.int32), out["fused"].view(torch.int32))),
               "x_megabytes": round(out["fused"].numel() * 4 / 1e6, 2)}
        rec["ratio_fused_over_calls"] = round(rec["fused"]["median_us"] / rec["calls"]["median_us"], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in recs)


if __name__ == "__main__":
    main()
