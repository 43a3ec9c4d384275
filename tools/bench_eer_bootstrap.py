#!/usr/bin/env python3
"""Times the bootstrap replicates of the empirical EER on the device (ops.eer_bootstrap, csrc/stats/eer_bootstrap.hip) against the host
form of the same arithmetic (tests/ref64_eer.py: Philox in numpy uint64, histogram and prefix sum per replicate, float64 numpy on this
machine's CPU), at

  1. n_tar = n_non = 18 860, m = 10 000      a VoxCeleb1-O sized list at feerci's default number of replicates
  2. n_tar = n_non = 2^20,   m = 1 000       the supported maximum per side
  3. n_tar = n_non = 100,    m = 10 000      a toy list: the one-wave-per-replicate form

The device side is the whole call with the cut tables already on the device: the launch and a device synchronisation.  The host side
is timed over `--host-replicates` replicates per window (fewer at 2^20) and EXTRAPOLATED linearly to m: replicates are independent and
cost the same, but it is an extrapolation, and the record says so.  Both sides run interleaved in every window; the median of
`--windows` windows and their spread (min .. max) are reported, after `--warmup` untimed calls of each side.  The replicates the host
side computed are compared with the device's: they must be equal.  Prints one JSON line per size; --out FILE also writes them to a file.

    python tools/bench_eer_bootstrap.py [--out profiles/eer_bootstrap_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref64_eer  # noqa: E402
import satools_amd  # noqa: E402,F401
from satools_amd import asv_eval, ops  # noqa: E402

DEV = "cuda"
SIZES = [(18860, 10000, 5, 8), (1 << 20, 1000, 1, 1), (100, 10000, 20, 64)]       # (n per side, m, device calls per window, host replicates per window)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--host-replicates", type=int, default=None, help="host replicates per window (default: per size)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eer_bootstrap.py needs the GPU: a time taken elsewhere says nothing")
    recs = []
    for n, m, iters, host_reps in SIZES:
        host_reps = a.host_replicates or host_reps
        g = np.random.default_rng(n)
        tar, non = np.sort(g.normal(1, 1, n)), np.sort(g.normal(-1, 1, n))
        ct, cn = asv_eval.eer_cuts(tar, non)
        dct, dcn = torch.from_numpy(ct).to(DEV), torch.from_numpy(cn).to(DEV)
        out = {}

        def device():
            out["dev"] = ops.eer_bootstrap(dct, dcn, n, n, m, seed=0)

        def host():
            out["host"] = ref64_eer.replicates(tar, non, 0, host_reps, 0)

        for _ in range(a.warmup):
            device()
            host()
        t_dev, t_host = [], []
        for _ in range(a.windows):                        # interleaved: every window times both sides
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                device()
            torch.cuda.synchronize()
            t_dev.append((time.perf_counter() - t0) / iters * 1e3)
            t0 = time.perf_counter()
            host()
            t_host.append((time.perf_counter() - t0) / host_reps * 1e3)
        same = all(np.array_equal(out["dev"][i][:host_reps].cpu().numpy(), out["host"][i]) for i in range(2))
        eers = np.minimum(out["dev"][0].cpu().numpy() / n, out["dev"][1].cpu().numpy() / n)
        rec = {"measurement": "eer_bootstrap", "shape": {"n_tar": n, "n_non": n, "K": int(len(ct) - 1), "m": m},
               "windows": a.windows, "device_calls_per_window": iters,
               "device": {"median_ms": round(statistics.median(t_dev), 4), "min_ms": round(min(t_dev), 4), "max_ms": round(max(t_dev), 4)},
               "host_per_replicate": {"median_ms": round(statistics.median(t_host), 4), "min_ms": round(min(t_host), 4), "max_ms": round(max(t_host), 4),
                                      "replicates_per_window": host_reps},
               "host_extrapolated_to_m_ms": round(statistics.median(t_host) * m, 1),
               "note": f"host time measured over {host_reps} replicates per window and extrapolated linearly to m = {m}",
               "replicates_equal": bool(same),
               "interval_95": [round(float(x), 6) for x in np.percentile(eers, [2.5, 97.5])]}
        rec["ratio_host_over_device"] = round(rec["host_extrapolated_to_m_ms"] / rec["device"]["median_ms"], 1)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        if not same:
            raise SystemExit("the host replicates differ from the device's")
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in recs))


if __name__ == "__main__":
    main()
