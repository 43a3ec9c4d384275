#!/usr/bin/env python3
"""Times the ASV scoring kernels against the same computation written with torch on the same device, the way the reference
writes it (scoring/__init__.py asnorm: einsum -> topk(200) -> mean / std, per TRIAL).

  1. cohort_topk_stats at N = 4096, C = 5994, D = 192, k = 200   vs  einsum + topk + mean + std of the same N rows
     (and at D = 4: the launch with next to no score phase, i.e. its selection and moment sweeps)
  2. the scoring of a VoxCeleb1-O sized list (37 720 trials, 4 715 enrolment vectors, 4 708 test utterances, 5 994 cohort rows):
     asv_eval.score_trials (statistics per unique vector, gathered per trial)  vs  the per-trial torch composition
  3. the whole of asv_eval.compute_metrics for that list (scoring, the `scores` file, the float64 metrics on the host), and
     its scoring and host-metric parts alone, in the same windows

Both sides of a pair run interleaved in every window; a window is `--iters` calls between two device synchronisations; the median
of `--windows` windows and their spread (min .. max) are reported, after `--warmup` untimed calls of each side.  Peak memory is the
device allocator's high-water mark over one call, above what was allocated before it.  Outputs of the two sides are compared.
Prints one JSON line per measurement; --out FILE also writes them to a file.

    python tools/bench_asv_score.py [--out profiles/asv_score_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import satools_amd  # noqa: E402,F401
from satools_amd import asv_eval, ops  # noqa: E402

DEV = "cuda"


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def torch_topk_stats(x, cohort, k):
    top = torch.einsum("ij,kj", x, cohort).topk(k, dim=1).values
    return top.mean(dim=1), top.std(dim=1)


def torch_per_trial(enroll, test, ie, it, cohort, k):
    """the reference's order of work: one enrolment and one test vector per trial, repeats included"""
    e, t = enroll[ie], test[it]
    s = torch.nn.functional.cosine_similarity(e, t, dim=1)
    me, se = torch_topk_stats(e, cohort, k)
    mt, st = torch_topk_stats(t, cohort, k)
    return s, 0.5 * ((s - me) / se + (s - mt) / st)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def compare(name, sides, warmup, windows, iters, extra=None):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():                   # interleaved: every window times every side
            times[k].append(window(fn, iters))
    rec = {"measurement": name, "windows": windows, "iters_per_window": iters}
    for k, v in times.items():
        rec[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "peak_device_MiB": round(peak_mb(sides[k]), 2)}
    keys = list(sides)
    if len(keys) == 2:
        rec[f"ratio_{keys[1]}_over_{keys[0]}"] = round(rec[keys[1]]["median_ms"] / rec[keys[0]]["median_ms"], 3)
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_asv_score.py needs the GPU: a time taken elsewhere says nothing")
    g = torch.Generator().manual_seed(0)
    N, C, D, k = 4096, 5994, 192, 200
    centres = torch.randn(64, D, generator=g)
    x = unit(centres[torch.arange(N) % 64] + 0.7 * torch.randn(N, D, generator=g)).to(DEV)
    cohort = unit(centres[torch.arange(C) % 64] + 1.5 * torch.randn(C, D, generator=g)).to(DEV)
    recs = []
    m0, s0 = ops.cohort_topk_stats(x, cohort, k)
    m1, s1 = torch_topk_stats(x, cohort, k)
    diff = {"max_abs_diff_mean": float((m0 - m1).abs().max()), "max_abs_diff_std": float((s0 - s1).abs().max()),
            "flop": 2 * N * C * D, "shape": {"N": N, "C": C, "D": D, "k": k}}
    recs.append(compare("cohort_topk_stats", {"hip": lambda: ops.cohort_topk_stats(x, cohort, k), "torch": lambda: torch_topk_stats(x, cohort, k)},
                        a.warmup, a.windows, a.iters, diff))
    # the same launch at D = 4: 1 / 48 of the products and of the cohort bytes, the same selection and moment sweeps — what the
    # launch costs apart from its score phase
    x4, c4 = x[:, :4].contiguous(), cohort[:, :4].contiguous()
    recs.append(compare("cohort_topk_stats_D4_selection_proxy", {"hip": lambda: ops.cohort_topk_stats(x4, c4, k), "torch": lambda: torch_topk_stats(x4, c4, k)},
                        a.warmup, a.windows, a.iters, {"shape": {"N": N, "C": C, "D": 4, "k": k}}))

    E, T, M = 4715, 4708, 37720
    enroll = unit(centres[torch.arange(E) % 64] + 0.7 * torch.randn(E, D, generator=g))
    test = unit(centres[torch.arange(T) % 64] + 0.9 * torch.randn(T, D, generator=g))
    ie = torch.randint(0, E, (M,), generator=g)
    it = torch.randint(0, T, (M,), generator=g)
    u2e = {f"e{i}": enroll[i].to(DEV) for i in range(E)}
    u2t = {f"t{j}": test[j].to(DEV) for j in range(T)}
    spk2utt = {f"s{i}": [f"e{i}"] for i in range(E)}
    spk, utt = [f"s{int(i)}" for i in ie], [f"t{int(j)}" for j in it]
    de, dt, die, dit = enroll.to(DEV), test.to(DEV), ie.to(DEV), it.to(DEV)
    ours = lambda: asv_eval.score_trials(u2e, u2t, spk2utt, spk, utt, cohort=cohort, device=torch.device(DEV))
    theirs = lambda: [v.cpu() for v in torch_per_trial(de, dt, die, dit, cohort, k)]
    a_s, a_as = ours()
    b_s, b_as = theirs()
    diff = {"max_abs_diff_score": float(np.abs(a_s - b_s.numpy()).max()), "max_abs_diff_asnorm": float(np.abs(a_as - b_as.numpy()).max()),
            "shape": {"trials": M, "enrol": E, "test": T, "C": C, "D": D, "k": k},
            "note": "hip side includes stacking 9 423 vectors from the dicts and the index lists on the host; torch side starts from device matrices"}
    recs.append(compare("score_trials_37720", {"hip": ours, "torch_per_trial": theirs}, 2, a.windows, max(1, a.iters // 10), diff))

    with tempfile.TemporaryDirectory() as d:
        trials = os.path.join(d, "trials")
        with open(trials, "w") as f:
            f.write("".join(f"{s} {u} {'target' if (int(s[1:]) % 64) == (int(u[1:]) % 64) else 'nontarget'}\n" for s, u in zip(spk, utt)))
        whole = lambda: asv_eval.compute_metrics(u2e, u2t, spk2utt, trials, d, cohort=cohort, device=torch.device(DEV))
        lab = np.asarray(["target" if (int(s[1:]) % 64) == (int(u[1:]) % 64) else "nontarget" for s, u in zip(spk, utt)]) == "target"
        sc, sc_as = ours()

        def host_metrics():
            asv_eval.score_metrics(sc[lab].astype(np.float64), sc[~lab].astype(np.float64))
            asv_eval.score_metrics(sc_as[lab].astype(np.float64), sc_as[~lab].astype(np.float64))

        # the whole call and its two parts, each warmed up and timed in the same interleaved windows
        recs.append(compare("compute_metrics_37720", {"whole": whole, "scoring_part": ours, "host_metrics_part": host_metrics}, 2,
                            min(a.windows, 7), 1))
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in recs))


if __name__ == "__main__":
    main()
