#!/usr/bin/env python3
"""Times the long form of YAAPT (f0.yaapt_long, csrc/yaapt_long/) against the resident form (f0.yaapt, one block's LDS per utterance) where
both run, and alone beyond it:

  1. 2048 frames (655 360 samples), B = 1 and B = 32      resident and long, alternated call by call inside every window
  2. 4097, 8193 frames and the cap (26 211 frames), B = 1  the long form alone

A timed call is the whole Python call (plan, workspace allocation, the launches) and a device synchronisation; the status word is
deferred and checked once after the windows.  After `--warmup` untimed calls of each side, the median of `--windows` windows and their
spread (min .. max) are reported.  At 2048 frames the two tracks must be equal bit for bit.  Prints one JSON line per size; --out FILE also
writes them to a file.

--opts NAME runs an option set by name instead of the anonymizer's options: a set of tests/yaapt_wide_cases.py (`defaults`: the
reference's default options, a 10 ms hop, frames three deep; `ov129`, `d2_even`, `d7`) or of tests/yaapt_cases.py.  A set the resident form
refuses (an overlap above 128 samples) is timed on the long form alone.  --shapes BxN[,BxN..] replaces the sizes above (e.g. 32x80000,1x327681).

    python tools/bench_yaapt_long.py [--opts defaults] [--shapes 32x80000,1x327681] [--out profiles/yaapt_long_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import satools_amd  # noqa: E402,F401
import yaapt_cases as yc  # noqa: E402
from satools_amd import f0 as f0_hip  # noqa: E402

DEV = "cuda"
CAP_FRAMES = 26211
SIZES = [(2048 * 320, 1, 5, True), (2048 * 320, 32, 2, True), (1310721, 1, 3, False), (2621441, 1, 2, False), (CAP_FRAMES * 320, 1, 1, False)]


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def option_set(name):
    """-> the options of the set `name`: "anonymizer" (tests/yaapt_cases.py OPTS), a wide set, or an option set of tests/yaapt_cases.py"""
    import yaapt_wide_cases as ywc
    if name == "anonymizer":
        return yc.OPTS
    for s in list(ywc.SETS) + list(yc.OPTION_SETS):
        if s.name == name:
            return s.opts
    raise SystemExit(f"no option set named {name!r}: anonymizer, {', '.join(s.name for s in list(ywc.SETS) + list(yc.OPTION_SETS))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opts", default="anonymizer", help="option set by name (tests/yaapt_wide_cases.py, tests/yaapt_cases.py)")
    ap.add_argument("--shapes", default=None, help="BxN[,BxN..] instead of the built-in sizes")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--chunk-frames", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_yaapt_long.py needs the GPU: a time taken elsewhere says nothing")
    opts = option_set(a.opts)
    resident_ok = f0_hip.plan_overlap(opts) <= f0_hip.MAX_RESIDENT_OVERLAP
    sizes = SIZES
    if a.shapes:
        sizes = [(int(n), int(B), 2, True) for B, n in (w.split("x") for w in a.shapes.split(","))]
    recs = []
    for n, B, iters, both in sizes:
        both = both and resident_ok and f0_hip.plan_frames(n, opts) <= f0_hip.MAX_RESIDENT_FRAMES
        row = yc.noisy_tone(1, n)
        wav = torch.stack([row.roll(1000 * b) for b in range(B)]).to(DEV)
        out = {}

        def resident():
            out["resident"], out["st_resident"] = f0_hip.yaapt(wav, opts, defer_status=True)

        def long():
            out["long"], out["st_long"] = f0_hip.yaapt_long(wav, opts, chunk_frames=a.chunk_frames, defer_status=True)

        sides = [("resident", resident), ("long", long)] if both else [("long", long)]
        for _ in range(a.warmup):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in sides}
        for _ in range(a.windows):
            spent = {name: 0.0 for name, _ in sides}
            for _ in range(iters):                      # alternated call by call: both sides see the same clocks
                for name, fn in sides:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    spent[name] += time.perf_counter() - t0
            for name in spent:
                times[name].append(spent[name] / iters * 1e3)
        for name, _ in sides:
            out["st_" + name].check()
        frames = out["long"].shape[1]
        rec = {"measurement": "yaapt_long", "opts": a.opts, "shape": {"B": B, "samples": n, "frames": frames}, "chunk_frames": a.chunk_frames or f0_hip.LONG_DEFAULT_CHUNK,
               "windows": a.windows, "calls_per_window": iters, "long": stats(times["long"]),
               "voiced_frames": int((out["long"] > 0).sum())}
        rec["long_us_per_frame"] = round(rec["long"]["median_ms"] * 1e3 / (B * frames), 3)
        if both:
            rec["resident"] = stats(times["resident"])
            rec["tracks_equal"] = bool(torch.equal(out["long"].view(torch.int32), out["resident"].view(torch.int32)))
            rec["ratio_long_over_resident"] = round(rec["long"]["median_ms"] / rec["resident"]["median_ms"], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        if both and not rec["tracks_equal"]:
            raise SystemExit("the long form's track differs from the resident form's")
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in recs))


if __name__ == "__main__":
    main()
