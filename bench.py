#!/usr/bin/env python3
"""Benchmark of the anonymize / model.convert() hot path on MI355X.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A "step" = one `model.convert` over one batch of 32 synthetic 5 s @ 16 kHz utterances per rank, everything on
the path (YAAPT F0, bottleneck extractor, one-hot, generator), inputs resident in HBM.  Rank 0 prints ONE JSON line
on stdout: the headline (BASELINE configs[1]: tag hifigan_bn_tdnnf_600h_vq_48_v1).

A plain run measures the headline alone: set-up, W warm-up steps, ONE timed window of exactly K steps
(`ms_per_step` = that window / K), then the line.  `--dump-outputs DIR` writes what the last timed step's convert()
returned (the anonymized waveforms, [32, 1, 80001] float32) to DIR/convert_y.npy; the inputs and the seeded weights are
the same in every run with the same arguments, so two builds can be compared output for output.

`--full` measures everything else as well: the headline becomes the median of `--repeats` windows (default 5) with
its `roofline` and `cpu_baseline`, and the other BASELINE configs are measured in the same run, before it; their
full lines (same schema) go to stderr prefixed `CONFIG_LINE ` and their value / roofline / cpu_baseline, condensed,
into the headline's `configs` object:

  N = 1   configs[2] (wav2vec2 tag), configs[3] (wav2vec2 tag + f0-transformation=quant_16_awgn_2), then the
          headline; each with its own `roofline` and `cpu_baseline`.
  N > 1   one process per GPU under torch.distributed (RCCL).  `python bench.py --gpus N` typed as is starts
          `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a CHILD process (the parent never
          touches the GPU) and relays its output and exit code; under the driver's own torch.distributed.run
          launch the ranks are used as they are.  Workload per line = the sharded job of SURVEY §8(d)/(e):
          N x K x 32 utterances, contiguous shards of K x 32 per rank, batches of 32 in index order
          (satools_amd.dist.convert_sharded), ONE all_gather_into_tensor of the [K*32, 1, 80001] shards at the
          end, inside the timed region.  With --full, BASELINE configs[4] (wav2vec2 tag; K = 16 at N = 8 is exactly
          its 4096 utterances) is measured first, then the headline tag through the same code (weak scaling: the
          per-GPU work is fixed, so the N = 1, 2, 4, 8 values are comparable).  --dump-outputs writes the last
          batch of the gathered job.

The CPU leg (`cpu_baseline`, --full, rank 0 at N = 1 only) times the oracle — a port of the reference's PyTorch CPU path —
on a bounded sample, at 1 thread (the reference's own setting, satools/satools/hifigan/yaapt.py:27) and at the
host's physical core count.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The path keeps several HIP streams busy per process (jobs in flight x (launch stream + YAAPT side
# stream)); the HIP runtime multiplexes streams onto 4 hardware queues by default, which serialises
# independent streams (measured 15.4 -> 14.3 ms/step at 2 jobs).  Must be set before the runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

TAG = "hifigan_bn_tdnnf_600h_vq_48_v1"
TAG_W2V2 = "hifigan_bn_tdnnf_wav2vec2_vq_48_v1"
BATCH = int(os.environ.get("SAT_BENCH_BATCH", "32"))      # BASELINE configs[1] is quoted at 32; other values are experiments (the line says which)
N_SAMPLES = 80000
UTT_SECONDS = 5.0
METRIC = "anonymized audio seconds per wall-clock second (real-time factor), 5 s @ 16 kHz utterances"
UNIT = "x real-time (audio s / wall s)"
# algorithmic work per 5 s utterance (SURVEY §8d / DESIGN.md §3)
GEN_FLOP_PER_UTT = 80.86e9          # generator: 40.43 GMAC
GEN_BYTES_PER_UTT = 731.4e6         # per-layer streaming model of the generator
W2V2_FLOP_PER_UTT = 185.5e9 + 0.92e9   # wav2vec2-large 92.73 GMAC + TDNNF tail 0.46 GMAC
W2V2_ACT_BYTES_PER_UTT = 620e6 + 5e6   # per-layer streaming model of the extractor's activations
W2V2_WEIGHT_BYTES = 1.26e9             # its weights, streamed once per batch
PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_F16_MFMA_TFLOPS = 2500.0       # dense f16/bf16 MFMA (MI355X_MICROARCH.md); split-f16 issues 3 MFMA products per product
PEAK_F8_MFMA_TFLOPS = 5000.0        # dense block-scaled e4m3 MFMA
# useful-FLOP peaks of the two split arithmetics: f16x3 = three f16 products per product; f16f8r = one f16 product + two e4m3
# products at twice the rate = two f16-product units per product
PEAK_F16X3 = PEAK_F16_MFMA_TFLOPS / 3.0
PEAK_F16F8R = 1.0 / (1.0 / PEAK_F16_MFMA_TFLOPS + 2.0 / PEAK_F8_MFMA_TFLOPS)
PEAK_HBM_TBS = 8.0
F0_OPTS = {"frame_length": 35.0, "frame_space": 20.0, "nccf_thresh1": 0.25, "tda_frame_length": 25.0}


# ---------------------------------------------------------------------------------------------------------
# CPU leg
# ---------------------------------------------------------------------------------------------------------
def host_cpu():
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        import psutil
        cores = psutil.cpu_count(logical=False) or os.cpu_count()
    except Exception:
        cores = os.cpu_count()
    try:
        cores = min(cores, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    return model, int(cores)


def cpu_baseline(tag, f0_transformation, spk, n_utt, runs_1, runs_n, n_utt_1=None, budget_note="", procs=0, n_utt_proc=0,
                 worker_mode=False):
    """the CPU oracle (a port of the reference's PyTorch path: serial YAAPT loop over the batch, fbank / wav2vec2,
    TDNNF-VQ, generator) timed on the host cores over a bounded sample of the same workload: one convert() batch of
    `n_utt` utterances, median of `runs_*` runs, at 1 thread and at the physical core count"""
    import torch
    from oracle import convert as oconv
    from oracle import f0 as of0
    from oracle import yaapt as oyaapt
    from satools_amd import f0_transforms, synthetic
    state, _ = synthetic.checkpoint(tag)
    sd = state["base_model_state_dict"]
    w2 = tag == TAG_W2V2
    omodel = None
    if w2:
        from oracle import wav2vec2 as ow
        omodel = ow.Wav2Vec2Restated(24)
        pfx = "bn_extractor.preprocessor."
        omodel.load_state_dict({k[len(pfx):]: v for k, v in sd.items() if k.startswith(pfx)})
        omodel.eval()
    quant = f0_transforms.parse_quant_bins(f0_transformation) if "quant" in f0_transformation else 0
    db = f0_transforms.parse_awgn_db(f0_transformation) if "awgn" in f0_transformation else None

    def once(seeds):
        wav = synthetic.harm_batch(seeds)
        tg = synthetic.targets(spk, seeds)
        with torch.no_grad():
            t0 = time.perf_counter()
            f0 = oyaapt.yaapt(wav, F0_OPTS)
            t1 = time.perf_counter()
            noise = f0_transforms.draw_awgn((len(seeds), 1, f0.shape[1]), db) if db is not None else None
            if w2:
                oconv.convert_w2v2(sd, spk, wav, tg, f0, quant, noise, model=omodel)
            else:
                oconv.convert_fbank(sd, spk, wav, tg, f0, quant, noise)
            t2 = time.perf_counter()
        return t2 - t0, t1 - t0

    if worker_mode:
        return once
    model_name, cores = host_cpu()
    keep = torch.get_num_threads()
    out = {"unit": UNIT, "kind": "port", "cpu_model": model_name}
    try:
        res = {}
        for label, threads, runs, n in (("threads1", 1, runs_1, n_utt_1 or n_utt), ("threadsN", cores, runs_n, n_utt)):
            torch.set_num_threads(threads)
            ts = [once(list(range(n))) for _ in range(runs)]
            dt = statistics.median(t[0] for t in ts)
            res[label] = {"value": round(n * UTT_SECONDS / dt, 3), "threads": threads, "utterances": n, "runs": runs,
                          "seconds": round(dt, 2), "yaapt_seconds": round(statistics.median(t[1] for t in ts), 2)}
    finally:
        torch.set_num_threads(keep)
    out.update(res)
    if procs > 0:
        # what the host can do the way the reference scales on CPUs: P single-thread PROCESSES side by side (its
        # jobs_per_compute_device model, bin/anonymize:85-93), each converting its own batch
        pr = cpu_processes(tag, f0_transformation, min(procs, max(1, cores)), n_utt_proc or n_utt)
        if pr:
            out["processes"] = res["processes"] = pr
    # `value` / `cores` = the fastest of the settings (what the host can do), all kept above
    best = max(res, key=lambda k: res[k]["value"])
    out["value"], out["cores"] = res[best]["value"], res[best]["threads"]
    out["sample"] = (f"one convert() batch, torch CPU f32: {res['threads1']['utterances']} x 5 s at 1 thread (the reference's "
                     f"setting, yaapt.py:27; median of {runs_1}) = {res['threads1']['value']} x RT in {res['threads1']['seconds']} s; "
                     f"{res['threadsN']['utterances']} x 5 s at {cores} threads (physical cores; median of {runs_n}) = "
                     f"{res['threadsN']['value']} x RT in {res['threadsN']['seconds']} s"
                     + (f"; {res['processes']['threads']} single-thread processes x {res['processes']['utterances_per_process']} x 5 s side by side = "
                        f"{res['processes']['value']} x RT in {res['processes']['seconds']} s" if "processes" in res else "") + budget_note)
    return out


def cpu_processes(tag, f0_transformation, procs, n_utt):
    """P child processes, one torch thread each, load the oracle, report READY, start together on GO and each convert one
    batch of n_utt utterances: throughput = P x n_utt x 5 s / the slowest process"""
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", tag, f0_transformation or "-", str(n_utt)]
    env = dict(os.environ, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    ps = []
    try:
        for i in range(procs):
            ps.append(subprocess.Popen(cmd + [str(i)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                       text=True, env=env))
        for p in ps:
            if p.stdout.readline().strip() != "READY":
                raise RuntimeError("cpu worker failed to load")
        for p in ps:
            p.stdin.write("GO\n")
            p.stdin.flush()
        secs = [float(p.stdout.readline()) for p in ps]
        for p in ps:
            p.wait(timeout=60)
    except Exception as e:                                   # the CPU leg is a reported baseline: never fail the bench on it
        for p in ps:
            p.kill()
        print(f"bench.py: process-parallel CPU leg skipped ({e})", file=sys.stderr)
        return None
    dt = max(secs)
    return {"value": round(procs * n_utt * UTT_SECONDS / dt, 3), "threads": procs, "processes": procs, "utterances_per_process": n_utt,
            "utterances": procs * n_utt, "runs": 1, "seconds": round(dt, 2), "slowest_fastest_process_s": [round(max(secs), 2), round(min(secs), 2)]}


def cpu_worker(tag, f0_tr, n_utt, index):
    import torch
    torch.set_num_threads(1)
    import satools_amd  # noqa: F401
    from satools_amd import synthetic
    state, _ = synthetic.checkpoint(tag)
    spk = sorted(set(state["base_model_params"]["utt2spk"].values()))
    once = cpu_baseline(tag, "" if f0_tr == "-" else f0_tr, spk, n_utt, 1, 1, worker_mode=True)
    print("READY", flush=True)
    sys.stdin.readline()
    dt, _ = once([index * n_utt + i for i in range(n_utt)])
    print(dt, flush=True)


# ---------------------------------------------------------------------------------------------------------
# GPU legs
# ---------------------------------------------------------------------------------------------------------
def load(tag, f0_transformation, dev):
    import satools_amd
    m = satools_amd.load_model("synthetic:" + tag, option_args={"f0_transformation": f0_transformation} if f0_transformation else None)
    m.to(dev)
    m.eval()
    return m


def run_steps(model, dev, rank, steps, warmup, jobs, seed_before_each, repeats=1, status="sync"):
    """N = 1 mode: K independent convert() batches, `jobs` deep in flight on separate HIP streams (the reference's
    jobs_per_compute_device, satools/satools/bin/anonymize:85-93), timed `repeats` times back to back (each window = exactly K steps
    between two device synchronisations).  Returns (list of window seconds, setup_steps, what the last timed step's convert() returned).
    status "sync" (default): the plain convert() call — YAAPT's status word of the batch (the error path: an utterance without a voiced
    frame) is waited for inside every call; "deferred": convert(..., defer_status=True), the word checked before the same job launches its
    NEXT batch and at the end of the window, as the batch job does (pipeline.process_data).  Measured level in this loop (8.91 / 8.93 /
    8.94 against 8.93 / 8.96 / 8.96 ms per step, interleaved on one box): what a 40-step window loses against the job's steady state is
    its fill and drain, not the round trip."""
    import torch
    from satools_amd import synthetic
    seeds = [rank * BATCH + i for i in range(BATCH)]
    wav = synthetic.harm_batch(seeds).to(dev)
    targets = synthetic.targets(model.spk, seeds)
    streams = [torch.cuda.Stream(device=dev) for _ in range(jobs)]
    # every job stream owns its workspaces and must have run (and allocated) once before the timed region starts: when
    # --warmup is smaller than the number of job streams, the missing runs are done as untimed set-up steps first
    setup_steps = max(0, jobs - warmup)
    n = [0]

    pending = [None] * jobs

    def step():
        j = n[0] % jobs
        n[0] += 1
        if seed_before_each:
            torch.manual_seed(1234)          # the awgn draw of every batch is reproducible
        if pending[j] is not None:
            pending[j].check()
            pending[j] = None
        with torch.cuda.stream(streams[j]):
            if status == "sync":
                return model.convert(wav, target=targets)
            y, pending[j] = model.convert(wav, target=targets, defer_status=True)
        # the batches launched in the previous steps: as soon as a batch's VQ launch has completed (a query, no wait) its near-tie
        # utterances (if any) go to the exact kernels on a side stream WITHOUT the launching thread waiting for them
        # (ConvertStatus.start; check() before the job's next batch finds them decided)
        for k in range(1, jobs):
            if pending[(j - k) % jobs] is not None:
                pending[(j - k) % jobs].start()
        return y

    def drain():
        for j in range(jobs):
            if pending[j] is not None:
                pending[j].check()
                pending[j] = None

    for _ in range(setup_steps + warmup):
        step()
    drain()
    windows = []
    chk = os.environ.get("SAT_BENCH_HOSTCHK") == "1"
    host_ms = []
    y = None
    for _ in range(max(1, repeats)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if chk:
                h0 = time.perf_counter()
                y = step()
                host_ms.append(1e3 * (time.perf_counter() - h0))
            else:
                y = step()
        drain()                              # every status of the window is checked inside it
        torch.cuda.synchronize()
        windows.append(time.perf_counter() - t0)
    if chk and host_ms:
        hs = sorted(host_ms)
        import gc
        print(f"HOSTCHK steps ({status}): host time per step mean {sum(hs) / len(hs):.2f} ms, median {hs[len(hs) // 2]:.2f}, p90 {hs[int(0.9 * len(hs))]:.2f}, "
              f"max {hs[-1]:.2f}; gc counts {gc.get_count()}, gen2 collections {gc.get_stats()[2]['collections']}", file=sys.stderr, flush=True)
    return windows, setup_steps, y


def run_sharded(model, dev, rank, world, steps, warmup, jobs, seed_before_each, gather="f32", repeats=1, chunk_batches=4, status="sync"):
    """N > 1 mode (and SAT_BENCH_FORCE_PG=1 with one rank): world x steps x 32 utterances sharded through
    satools_amd.dist.convert_sharded, all inside the timed region.  The exchange of the anonymized waveforms is issued in chunks of
    `chunk_batches` batches on a communication stream while the rest of the shard is computed (dist.ChunkedGather: the bytes of the
    one all_gather_into_tensor, hidden behind compute; `chunk_batches` = 0: that single collective at the end).
    `gather` = "pcm16": the shards are converted to the int16 PCM the reference writes before the collective (half the
    bytes).  The job is timed `repeats` times (each window: barrier + synchronize on both sides, MAX over ranks).
    Returns a dict: window seconds, exposed all-gather ms, per-rank compute ms, ranks seen, setup_steps, checks, the last batch of the
    gathered job."""
    import torch
    import torch.distributed as dist
    from satools_amd import dist as sdist
    from satools_amd import synthetic
    n_items = world * steps * BATCH
    lo, hi = sdist.shard_bounds(n_items, rank, world)
    # this rank's shard of utterances, resident in HBM (seeds = global utterance indices)
    wav = torch.cat([synthetic.harm_batch(list(range(s, e))) for s, e in sdist.batches(lo, hi, BATCH)], 0).to(dev)
    targets = synthetic.targets(model.spk, list(range(lo, hi)))
    streams = [torch.cuda.Stream(device=dev) for _ in range(jobs)]
    comm = torch.cuda.Stream(device=dev)
    local = torch.empty(hi - lo, 1, N_SAMPLES + 1, dtype=torch.float32, device=dev)
    setup_steps = max(0, jobs - warmup)
    cur = torch.cuda.current_stream(dev)
    n = [0]
    produced = {}           # first utterance of a batch -> event behind its last kernel
    pending = [None] * jobs  # status "deferred" (run_steps): YAAPT's status word of a job's batch, checked before its next batch and before the shard is joined

    def check_pending(j):
        # a deferred status may replace rows of y (near-tie utterances of the VQ decided again on the exact kernels): copied again
        if pending[j] is not None:
            st, y, a, b, s = pending[j]
            pending[j] = None
            st.check()
            if getattr(st, "rows", None):
                with torch.cuda.stream(s):
                    local[a - lo:b - lo].copy_(y.reshape(b - a, 1, -1))
                    e = torch.cuda.Event()
                    e.record(s)
                    produced[a] = e

    def convert_fn(a, b):
        s = streams[n[0] % jobs]
        n[0] += 1
        if seed_before_each:
            torch.manual_seed(1234)
        j = (n[0] - 1) % jobs
        check_pending(j)
        with torch.cuda.stream(s):
            if status == "sync":
                y = model.convert(wav[a - lo:b - lo], target=targets[a - lo:b - lo])
            else:
                y, st = model.convert(wav[a - lo:b - lo], target=targets[a - lo:b - lo], defer_status=True)
                pending[j] = (st, y, a, b, s)
            local[a - lo:b - lo].copy_(y.reshape(b - a, 1, -1))
            e = torch.cuda.Event()
            e.record(s)
            produced[a] = e
        if status != "sync":
            for k in range(1, jobs):                     # (run_steps: the near-tie utterances of the batches launched before, without waiting)
                if pending[(j - k) % jobs] is not None:
                    pending[(j - k) % jobs][0].start()
        return None

    def before_chunk(c, ra, rb):
        # the communication stream waits for the job streams that produced this chunk's batches; the collective is issued behind it
        for j in range(jobs):                      # (deferred statuses of the chunk's batches first: they may rewrite rows)
            if pending[j] is not None and lo + ra <= pending[j][2] < lo + rb:
                check_pending(j)
        for a in range(lo + ra, lo + rb, BATCH):
            comm.wait_event(produced[a])
        return torch.cuda.stream(comm)

    def join_streams():
        for j in range(jobs):
            check_pending(j)
        for s in streams:
            cur.wait_stream(s)
        ev[1].record(cur)           # this rank's compute is done
        cur.wait_stream(comm)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for i in range(setup_steps + warmup):
        convert_fn(lo + (i % steps) * BATCH, lo + (i % steps) * BATCH + BATCH)
    for j in range(jobs):
        check_pending(j)
    for s in streams:
        cur.wait_stream(s)
    transform = sdist.pcm16_rows if gather == "pcm16" else None
    ref = sdist.all_gather_rows(transform(local) if transform else local, n_items)   # first collective: RCCL builds its communicator / rings here
    ranks_seen = [torch.empty(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(ranks_seen, torch.tensor([rank], dtype=torch.int64, device=dev))
    ranks_seen = [int(t.item()) for t in ranks_seen]
    windows, gather_ms, compute_ms, stats, chunk_ms = [], [], [], {}, []
    out = None
    for _ in range(max(1, repeats)):
        del out
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record(cur)
        out = sdist.convert_sharded(convert_fn, n_items, BATCH, gather=True, local_out=local, before_gather=join_streams, transform=transform,
                                    gather_chunk_batches=chunk_batches, before_chunk=before_chunk if chunk_batches else None, stats=stats)
        ev[2].record(cur)
        torch.cuda.synchronize()
        dist.barrier()
        dt = time.perf_counter() - t0
        # per window: MAX over ranks of the wall time and of the exposed exchange; every rank's compute time (a straggler is visible)
        t = torch.tensor([dt, ev[1].elapsed_time(ev[2])], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        comp = [torch.empty(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(comp, torch.tensor([ev[0].elapsed_time(ev[1])], dtype=torch.float64, device=dev))
        windows.append(float(t[0].item()))
        gather_ms.append(float(t[1].item()))
        compute_ms.append([round(float(c.item()), 3) for c in comp])
        # per chunk of the exchange: host time of its issue and of the wait for it in finish(), MAX over ranks — a rank that delays a
        # chunk shows up at that chunk (dist.ChunkedGather.stats)
        ch = stats.get("chunks", []) if chunk_batches else []
        if ch:
            cw = torch.tensor([[c.get("issue_ms", 0.0), c.get("wait_ms", 0.0)] for c in ch], dtype=torch.float64, device=dev)
            dist.all_reduce(cw, op=dist.ReduceOp.MAX)
            chunk_ms.append([[round(float(v), 3) for v in row] for row in cw.tolist()])
    assert out.shape == (n_items, 1, N_SAMPLES + 1)
    mine = transform(local) if transform else local
    # the checked reference: ONE all_gather_into_tensor of the same shards (same inputs -> same waveforms as the warm-up pass it gathered)
    ref2 = sdist.all_gather_rows(mine, n_items)
    ok = torch.tensor([0.0 if torch.equal(out[lo:hi], mine) else 1.0, 0.0 if torch.equal(out, ref2) else 1.0], dtype=torch.float64, device=dev)
    dist.all_reduce(ok, op=dist.ReduceOp.MAX)
    del ref, ref2
    return {"windows": windows, "all_gather_ms": gather_ms, "compute_ms_per_rank": compute_ms, "ranks_seen": ranks_seen, "setup_steps": setup_steps,
            "gathered_equals_shard": ok[0].item() == 0.0, "chunked_equals_single_collective": ok[1].item() == 0.0,
            "chunks": len(stats.get("chunks", [])), "chunk_batches": chunk_batches, "chunk_issue_wait_ms": chunk_ms,
            "last_batch": out[n_items - BATCH:]}


def last_dispatch():
    """the kernel (family<template arguments>) the library launched last on this thread: read back, not assumed"""
    from satools_amd import _lib
    return _lib.lib().sat_last_dispatch_name().decode()


def time_events(fn, reps, warm=2, samples=5):
    """Per-call time of `fn` in ms from events on the launch stream: warmed until two successive batches of 5 calls agree
    within 3 % (at least `warm` calls, at most 10 batches: the first calls of a leg pay allocations, code loading and a cold
    clock), then the MEDIAN of `samples` timings of `reps` calls each.  Returns (median, {"min", "max", "samples", "warm_batches"})."""
    import torch

    def batch(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for _ in range(warm):
        fn()
    prev, batches = batch(5), 1
    while batches < 10:
        cur = batch(5)
        batches += 1
        if abs(cur - prev) <= 0.03 * min(cur, prev):
            break
        prev = cur
    ts = sorted(batch(max(1, reps)) for _ in range(samples))
    return ts[len(ts) // 2], {"min": round(ts[0], 4), "max": round(ts[-1], 4), "samples": samples, "calls_per_sample": max(1, reps), "warm_batches_of_5": batches}


def roofline_generator(model, dev, reps):
    """the generator (dominant on the fbank tag): all launches of one forward timed with events on the launch
    stream, and its dominant kernel alone"""
    import torch
    from satools_amd import ops, packing, synthetic
    seeds = list(range(BATCH))
    wav = synthetic.harm_batch(seeds).to(dev)
    targets = synthetic.targets(model.spk, seeds)
    with torch.no_grad():
        f0n = model.get_f0(wav)
        bn = model.get_bn(wav)
        spk = model.get_spk_id(wav, targets)
        ops.f0_norm_transform_(f0n)
        x = ops.assemble_input(bn, f0n, spk.to(dev, torch.float32).contiguous(), spk.shape[1])
        gen_ms, gen_t = time_events(lambda: model.hifigan(x), reps)
    prec = model.hifigan.precision
    split = prec in ("f16x3", "f16f8r")
    f8 = prec == "f16f8r" and bool(getattr(model.hifigan, "_packed8", None))
    dom = None
    if split:
        # The generator's thick stages launch ONE kernel per conv of the three MRF branches (hifigan.hip, option multi_branch): 12
        # launches of the LDS-DMA ring kernel per forward, 6 at C = 256 / T = 1250 and 6 at C = 128 / T = 5000.  Both shapes are
        # timed live (the second conv of a ResBlock step: 3 + 7 + 11 taps, residual from planes, planes out) and the one with the
        # larger TOTAL time per forward is reported as the dominant kernel (round 4 reported the C = 256 shape by fiat).
        cands = []
        for C, T in ((256, 1250), (128, 5000)):
            ks = (3, 7, 11)
            g = torch.Generator(device="cpu").manual_seed(0)
            xk = torch.randn(BATCH, C, T, generator=g).to(dev)
            xs, rs = ops.act_split(xk, 0.1), ops.act_split(xk * 0.5, 0.1)
            xs8 = ops.planes_f8_sidecar(xs) if f8 else None
            jobs = []
            for k in ks:
                wf = (torch.randn(C, C, k, generator=g) * 0.02).to(dev)
                wk = packing.pack_conv_weight_f16f8r(wf) if f8 else packing.pack_conv_weight_f16x3(wf)
                kw = dict(bias=torch.zeros(C, device=dev), dilation=1, pad_left=(k - 1) // 2, mode=3 if f8 else 1, x_split=xs,
                          y_split=ops.split_like(BATCH, C, T, dev), y_split_slope=0.1, res_split=rs, res_split_slope=0.1, no_y=True)
                if f8:
                    kw.update(x_split8=xs8, y_split8=ops.sidecar_like(BATCH, C, T, dev))
                jobs.append((xk, wk, C, k, kw))
            run = lambda: ops.conv1d_multi(jobs)
            us, us_t = time_events(run, 20, warm=3)
            us, us_t = us * 1e3, {k_: (round(v * 1e3, 1) if k_ in ("min", "max") else v) for k_, v in us_t.items()}
            flop = 2.0 * BATCH * C * C * sum(ks) * T
            peak_k = PEAK_F16F8R if f8 else PEAK_F16X3
            cands.append({"name": last_dispatch() + f" — one launch = the second conv (3 + 7 + 11 taps, residual from planes, planes out) of the three MRF "
                                                    f"branches at C={C}, T={T}, batch 32 (6 launches of this shape per forward)",
                          "launches_per_forward": 6, "total_us_per_forward": round(6 * us, 1),
                          "flop_per_launch": flop, "avg_us_per_launch": round(us, 1), "us_per_launch_min_max": us_t, "achieved": round(flop / us / 1e6, 1),
                          "peak": round(peak_k, 1), "frac": round(flop / us / 1e6 / peak_k, 4)})
            del xk, xs, rs, jobs
        cands.sort(key=lambda c: -c["total_us_per_forward"])
        dom = dict(cands[0], chosen_by="largest total time per forward among the generator's launch shapes timed live",
                   other_candidates=[{k_: c[k_] for k_ in ("name", "total_us_per_forward", "avg_us_per_launch", "achieved", "frac")} for c in cands[1:]])
    achieved = GEN_FLOP_PER_UTT * BATCH / (gen_ms * 1e-3) / 1e12
    _, peak, arithmetic = gen_arithmetic(model)
    hbm = GEN_BYTES_PER_UTT * BATCH / (gen_ms * 1e-3) / 1e12
    traffic, note = None, None
    for name in (["r06_generator_f16f8r_traffic.json", "r05_generator_f16f8r_traffic.json"] if f8 else []) + ["r06_generator_traffic.json", "r05_generator_traffic.json", "r04_generator_traffic.json", "r03_generator_traffic.json"]:
        tpath = os.path.join(ROOT, "profiles", name)
        if os.path.exists(tpath):
            tj = json.load(open(tpath))["per_forward"]
            # gfx950 counts a 128-byte request of a 16-byte-per-lane load as 64 bytes in FETCH_SIZE: these kernels
            # issue such loads, so the fetch figure is doubled (MI355X_MICROARCH.md, HBM)
            traffic = (tj["fetch_GB_doubled"] + tj["write_GB"]) * 1e9
            note = (f"HBM bytes per generator forward (batch 32), separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes "
                    f"(profiles/{name}): fetch {tj['fetch_GB_doubled']} GB (FETCH_SIZE x 2, the gfx950 wide-load correction) "
                    f"+ write {tj['write_GB']} GB; per-layer streaming model {tj['algorithmic_GB_per_layer_model']} GB"
                    + ("" if ("generator_f16f8r" in name or not f8) else " — counters of the f16x3 generator: the f16f8r forward also moves the e4m3 sidecars of the thick stages"))
            break
    return {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_note": note,
            # north_star's quantity for the upsample stack: counted HBM bytes of a forward / its measured time / the HBM peak
            "hbm_frac_counters": (round(traffic / (gen_ms * 1e-3) / 1e12 / PEAK_HBM_TBS, 4) if traffic else None),
            "kernel": (("split-f16 conv family of the generator" + (" (8-bit cross terms on the thick stages)" if f8 else "")) if split else "conv1d_mfma_kernel (exact f32)")
                      + f": all launches of one forward, {gen_ms:.3f} ms per batch of {BATCH}",
            "timing_ms": dict(gen_t, median=round(gen_ms, 4)),
            "dominant_kernel": dom,
            "arithmetic": arithmetic,
            "algorithmic_flop_per_launch_group": GEN_FLOP_PER_UTT * BATCH,
            "hbm_model": {"achieved_TBps": round(hbm, 3), "peak_TBps": PEAK_HBM_TBS, "frac": round(hbm / PEAK_HBM_TBS, 4),
                          "bytes_per_launch_group": GEN_BYTES_PER_UTT * BATCH}}


def roofline_w2v2(model, dev, reps):
    """the wav2vec2 bottleneck extractor (dominant on the wav2vec2 tag, ~2/3 of a step): all its launches timed with
    events, and its dominant kernel (the 1x1 GEMM of the 146 Linear layers) alone on the FFN shape"""
    import torch
    from satools_amd import ops, packing, synthetic
    wav = synthetic.harm_batch(list(range(BATCH))).to(dev)
    with torch.no_grad():
        ext_ms, ext_t = time_events(lambda: model.get_bn(wav), reps)
        cin, cout, T = 1024, 4096, 249
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(BATCH, cin, T, generator=g).to(dev)
        w = packing.pack_conv_weight_f16x3((torch.randn(cout, cin, 1, generator=g) * 0.03).to(dev))
        b = torch.zeros(cout, device=dev)
        xs, ys = ops.act_split(x, 1.0), ops.split_like(BATCH, cout, T, dev)
        run = lambda: ops.conv1d(x, w, cout, 1, bias=b, gelu=True, mode=1, x_split=xs, y_split=ys, y_split_slope=1.0, no_y=True)
        us, us_t = time_events(run, 20, warm=3)
        us, us_t = us * 1e3, {k_: (round(v * 1e3, 1) if k_ in ("min", "max") else v) for k_, v in us_t.items()}
        dom_name = last_dispatch()
    flop = 2.0 * BATCH * T * cin * cout
    peak = PEAK_F16_MFMA_TFLOPS / 3.0
    achieved = W2V2_FLOP_PER_UTT * BATCH / (ext_ms * 1e-3) / 1e12
    model_bytes = W2V2_ACT_BYTES_PER_UTT * BATCH + W2V2_WEIGHT_BYTES
    hbm = model_bytes / (ext_ms * 1e-3) / 1e12
    traffic, note = None, None
    for tname in ("r06_w2v2_traffic.json", "r04_w2v2_traffic.json", "r03_w2v2_traffic.json"):
        tpath = os.path.join(ROOT, "profiles", tname)
        if not os.path.exists(tpath):
            continue
        tj = json.load(open(tpath))["per_forward"]
        traffic = (tj["fetch_GB_doubled"] + tj["write_GB"]) * 1e9
        note = (f"HBM bytes per get_bn() of a batch of 32, separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes "
                f"(profiles/{tname}): fetch {tj['fetch_GB_doubled']} GB (FETCH_SIZE x 2, the gfx950 wide-load "
                f"correction) + write {tj['write_GB']} GB; per-layer streaming model {model_bytes / 1e9:.2f} GB")
        break
    return {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_note": note,
            "hbm_frac_counters": (round(traffic / (ext_ms * 1e-3) / 1e12 / PEAK_HBM_TBS, 4) if traffic else None),
            "hbm_model": {"achieved_TBps": round(hbm, 3), "peak_TBps": PEAK_HBM_TBS, "frac": round(hbm / PEAK_HBM_TBS, 4),
                          "bytes_per_launch_group": model_bytes},
            "kernel": f"wav2vec2-large + TDNNF tail bottleneck extractor (get_bn): all launches, {ext_ms:.3f} ms per batch of {BATCH}",
            "timing_ms": dict(ext_t, median=round(ext_ms, 4)),
            "dominant_kernel": {"name": dom_name + " — the 1x1 GEMM on split planes of the encoder's Linear layers: FFN 1024 -> 4096 + GELU, 249 frames, batch 32",
                                "flop_per_launch": flop, "avg_us_per_launch": round(us, 1), "us_per_launch_min_max": us_t, "achieved": round(flop / us / 1e6, 1),
                                "frac": round(flop / us / 1e6 / peak, 4)},
            "arithmetic": "f32 operands split hi+lo f16, 3 f16 MFMA products per product, f32 accumulate; peak = dense f16 MFMA peak / 3",
            "algorithmic_flop_per_launch_group": W2V2_FLOP_PER_UTT * BATCH}


def aux_forwards(dev):
    """SURVEY 8 f3 / f4 — the forwards beside the anonymization path that are built and parity-tested but are not BASELINE configs:
    the x-vector extractor (ECAPA-TDNN, egs/asv/voxceleb/local/tuning/ecapa_tdnn.py:36-81) and the full ASR forward up to the
    chain / xent log-likelihoods of both bottleneck nets (tdnnf_vq.py:259-284, tdnnf_wav2vec2_vq.py:316-345), batch 32 x 5 s,
    timed with events on the launch stream (median of five timings of ten calls, warmed like every roofline leg)."""
    import torch
    from satools_amd import synthetic, xvector
    import satools_amd
    out = {}
    wav = synthetic.harm_batch(list(range(BATCH))).to(dev)
    rt = lambda ms: round(BATCH * UTT_SECONDS / (ms * 1e-3), 1)
    with torch.no_grad():
        net = xvector.build()(num_speakers=10)
        net.load_state_dict(synthetic.xvector_state(0, 10))
        net = net.to(dev)
        ms, t = time_events(lambda: net(wav), 10)
        out["f3 x-vector extractor"] = {"workload": "ECAPA-TDNN x-vector extractor forward (MelSpectrogram front end included), batch 32 x 5 s, " + str(net.precision),
                                        "value": rt(ms), "unit": "x real-time", "ms_per_batch": round(ms, 3), "timing_ms": t}
        del net
        for name, tag in (("f4 ASR forward (fbank tag)", TAG), ("f4 ASR forward (wav2vec2 tag)", TAG_W2V2)):
            model = load(tag, "", dev)
            ext = model.bn_extractor
            ms, t = time_events(lambda: ext(wav.clone()), 10)          # (the fbank net scales its argument in place, like the reference)
            out[name] = {"workload": f"Net.forward of the bottleneck net of {tag} up to the chain / xent log-likelihoods, batch 32 x 5 s, {ext.precision}",
                         "value": rt(ms), "unit": "x real-time", "ms_per_batch": round(ms, 3), "timing_ms": t}
            del model, ext
            torch.cuda.empty_cache()
    return out


def gen_arithmetic(model):
    """(dtype string, useful-FLOP peak in TFLOP/s, description) of what the generator's matrix products run as — read from the
    loaded model (precision + the stages whose second packing is installed), not assumed"""
    g = model.hifigan
    if g.precision == "f32":
        return "f32", PEAK_F32_MFMA_TFLOPS, "exact f32 MFMA"
    if g.precision == "f16f8r" and getattr(g, "_packed8", None):
        # FLOP share of the ResBlock convs that run with e4m3 cross terms (batch 32: the ring kernel serves them): per stage
        # C^2 T (3 + 7 + 11) x 6 convs MACs (hifigan/archi.py:82-86)
        n_ups, nk = len(g.upsample_rates), len(g.resblock_kernel_sizes)
        C, T, f8 = g.upsample_initial_channel, 250, 0.0
        stages = {(int(i) - 1 - n_ups) // (6 * nk) for i in g._packed8}
        for i, u in enumerate(g.upsample_rates):
            C, T = C // 2, T * u
            if i in stages:
                f8 += 2.0 * C * C * T * sum(g.resblock_kernel_sizes) * 6
        share = f8 / GEN_FLOP_PER_UTT
        peak = 1.0 / (share / PEAK_F16F8R + (1.0 - share) / PEAK_F16X3)
        return (f"f32 (matrix products as split-f16: hi*hi on the f16 MFMA; cross terms on the block-scaled 8-bit MFMA (weights e4m3, activations e5m2) in the ResBlock convs of stages "
                f"{sorted(s + 1 for s in stages)} = {100 * share:.0f} % of the generator's FLOP, as two more f16 products elsewhere; f32 accumulate)",
                peak, f"split-f16; {100 * share:.0f} % of the FLOP at 2 f16-product units per product (f16 + 2 x 8-bit at twice the rate: peak "
                      f"{PEAK_F16F8R:.0f}), the rest at 3 (peak {PEAK_F16X3:.0f}): FLOP-weighted harmonic peak")
    if g.precision == "f16x3":
        return "f32 (matrix products as split-f16 x3 with f32 accumulate)", PEAK_F16X3, "f32 operands split hi+lo f16, 3 f16 MFMA products per product, f32 accumulate; peak = dense f16 MFMA peak / 3"
    return f"f32 (matrix products: {g.precision})", PEAK_F16X3, g.precision


def dump_outputs(outdir, arrays):
    """what the timed path returned, as float32 .npy files in `outdir`, at most 64 MB in all: a larger array keeps a fixed, seeded
    sample of its rows (leading dimension)"""
    import numpy as np
    import torch
    os.makedirs(outdir, exist_ok=True)
    budget = 64 * 2 ** 20 // max(1, len(arrays))
    for name, t in arrays.items():
        t = t.detach().float().cpu()
        row = max(1, t[0].numel() * 4)
        if t.numel() * 4 > budget:
            keep = torch.randperm(t.shape[0], generator=torch.Generator().manual_seed(0))[:max(1, budget // row)].sort().values
            t = t[keep]
        np.save(os.path.join(outdir, name + ".npy"), t.numpy())


def one_config(name, tag, f0_tr, a, dev, rank, world, use_pg, steps, warmup, want_cpu, cpu_args, repeats=1, gen_precision=None, want_roofline=True, status=None,
               dump=None):
    """measure one BASELINE config on the loaded device; returns the JSON object (rank 0) or None.  `value` = the MEDIAN of
    `repeats` timed windows of `steps` steps (median of >= 5 repeats), min / max beside it.  `dump`: a directory that
    receives what the last timed step computed (dump_outputs), written before anything else runs on the model."""
    model = load(tag, f0_tr, dev)
    if gen_precision:
        model.hifigan.precision = gen_precision
        model.hifigan.invalidate()
    seed_each = "awgn" in f0_tr
    extra = {}
    status = status or a.f0_status
    if use_pg:
        r = run_sharded(model, dev, rank, world, steps, warmup, a.jobs, seed_each, a.gather, repeats, a.gather_chunk, status=status)
        windows, setup, y = r["windows"], r["setup_steps"], r["last_batch"]
        gb = 2 if a.gather == "pcm16" else 4
        mid = sorted(range(len(windows)), key=lambda i: windows[i])[len(windows) // 2]
        comp = r["compute_ms_per_rank"][mid]
        extra = {"all_gather_ms": round(r["all_gather_ms"][mid], 3), "ranks_seen_by_rccl": r["ranks_seen"],
                 "utterances": world * steps * BATCH, "gather_dtype": "int16" if a.gather == "pcm16" else "float32",
                 "gathered_equals_shard": r["gathered_equals_shard"], "chunked_equals_single_collective": r["chunked_equals_single_collective"],
                 "compute_ms_per_rank": comp, "compute_ms_min_max": [min(comp), max(comp)],
                 "chunk_issue_wait_ms_max_over_ranks": (r["chunk_issue_wait_ms"][mid] if r["chunk_issue_wait_ms"] else None),
                 "all_gather": (f"{r['chunks']} asynchronous all-gathers of {r['chunk_batches']} batches each ([{r['chunk_batches'] * BATCH}, 1, {N_SAMPLES + 1}] "
                                if r["chunk_batches"] else f"one all_gather_into_tensor of [{steps * BATCH}, 1, {N_SAMPLES + 1}] ")
                               + f"{'int16 PCM' if a.gather == 'pcm16' else 'f32'} per rank; {steps * BATCH * (N_SAMPLES + 1) * gb / 1e6:.0f} MB per rank in all), "
                               + ("issued on a communication stream as the batches complete, inside the timed region; all_gather_ms = what is left "
                                  "exposed behind the slowest rank's last batch" if r["chunk_batches"] else "at the end, inside the timed region")}
    else:
        windows, setup, y = run_steps(model, dev, rank, steps, warmup, a.jobs, seed_each, repeats, status=status)
    if dump and rank == 0:
        dump_outputs(dump, {"convert_y": y})
    del y
    ext = model.bn_extractor
    tie = dict(ext.__dict__.get("tie_stats") or {})
    if rank != 0:
        return None
    w2 = tag == TAG_W2V2
    reps = max(3, min(steps, 10))
    dt = statistics.median(windows) if len(windows) % 2 else sorted(windows)[len(windows) // 2]
    dtype, _, _ = gen_arithmetic(model)
    val = lambda t: round(world * steps * BATCH * UTT_SECONDS / t, 2)
    out = {"metric": METRIC, "value": val(dt), "unit": UNIT, "n_gpus": world,
           "steps": steps, "warmup": warmup, "ms_per_step": round(dt / steps * 1e3, 3), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None,
           "dtype": dtype, "data": "synthetic",
           "repeats": {"windows": len(windows), "steps_per_window": steps, "value": "median window", "value_min_max": [val(max(windows)), val(min(windows))],
                       "ms_per_step_windows": [round(t / steps * 1e3, 3) for t in windows]},
           "config": dict({"workload": f"{name}: {tag}{'+f0-transformation=' + f0_tr if f0_tr else ''} model.convert, "
                                       f"batch=32 x 5 s @ 16 kHz synthetic `harm` utterances per GPU",
                           "batch_per_gpu": BATCH, "utt_seconds": UTT_SECONDS, "weights": "seeded random (conditioned)",
                           "f0": "YAAPT computed on-path on the GPU inside convert()", "jobs_per_gpu": a.jobs,
                           "f0_status": ("convert(..., defer_status=True), as the batch job does (pipeline.process_data): a batch's deferred work — YAAPT's status word "
                                         "(convert()'s error path) and the utterances whose VQ decision was a near-tie, decided again on the exact kernels — is "
                                         "checked before the same job launches its next batch and at the end of every timed window, inside the timed region"
                                         if status == "deferred" else "the plain convert() call: status word and near-tie utterances waited for inside every call (host round trips to the GPU per step)"),
                           "vq_near_tie_guard": {"window_sigmas": getattr(ext, "vq_tie_sigmas", None), "utterances": tie.get("utterances"),
                                                 "decided_again_on_exact_kernels": tie.get("rerun"), "changed_and_generated_again": tie.get("changed")},
                           "setup_steps": setup, "generator_precision": model.hifigan.precision,
                           "reference_default_tag": f"{TAG_W2V2} (hubconf.py:69): its lines are configs[2] / configs[3] / configs[4] of this same run; "
                                                    f"the headline is BASELINE.json's configs[1], the tag the metric is quoted on",
                           "parallelism": f"dp{world}" + (" sharded (contiguous shards, batches of 32 in index order)" if use_pg else "")},
                          **extra)}
    if os.environ.get("SAT_BENCH_HOSTCHK") == "1":
        # diagnostic: how long the launching thread needs to ENQUEUE ten generator forwards in this process state (no device wait)
        import torch
        xg = torch.randn(BATCH, model.hifigan.imput_dim, 250, device=dev)
        model.hifigan(xg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            model.hifigan(xg)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(f"HOSTCHK {name}: enqueue of 10 generator forwards {1e3 * (t1 - t0):.1f} ms, until done {1e3 * (t2 - t0):.1f} ms; "
              f"threads {torch.get_num_threads()}", file=sys.stderr, flush=True)
    if want_roofline:
        out["roofline"] = roofline_w2v2(model, dev, reps) if w2 else roofline_generator(model, dev, reps)
    if want_cpu:
        out["cpu_baseline"] = cpu_baseline(tag, f0_tr, model.spk, **cpu_args)
    del model
    return out


def dryrun(a, rank, world):
    """SAT_BENCH_DRYRUN=1 (CPU tests): the launch plumbing and the sharded job without a GPU — gloo ranks, the same
    convert_sharded call as run_sharded (preallocated shard buffer filled by the callback, pre-gather hook, one
    all-gather), a stand-in convert() whose rows carry their global utterance index"""
    import torch
    import torch.distributed as dist
    from satools_amd import dist as sdist
    dist.init_process_group("gloo")
    assert dist.get_world_size() == world == a.gpus, (dist.get_world_size(), world, a.gpus)
    n_items = world * a.steps * BATCH
    lo, hi = sdist.shard_bounds(n_items, rank, world)
    local = torch.full((hi - lo, 1, 5), -1.0)
    calls, hooked = [], []

    def convert_fn(s, e):
        calls.append((s, e))
        local[s - lo:e - lo] = torch.arange(s, e, dtype=torch.float32).view(-1, 1, 1)

    t0 = time.perf_counter()
    out = sdist.convert_sharded(convert_fn, n_items, BATCH, gather=True, local_out=local, before_gather=lambda: hooked.append(1))
    dt = time.perf_counter() - t0
    assert hooked == [1] and calls == sdist.batches(lo, hi, BATCH) and len(calls) == a.steps
    assert out.shape == (n_items, 1, 5) and torch.equal(out[:, 0, 0], torch.arange(n_items, dtype=torch.float32))
    dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": round(n_items * UTT_SECONDS / dt, 2), "unit": UNIT, "n_gpus": world,
                          "steps": a.steps, "warmup": a.warmup, "data": "dry run (CPU, gloo, stand-in convert)",
                          "config": {"workload": "dry run of the sharded job", "utterances": n_items, "parallelism": f"dp{world}"}}), flush=True)
    dist.destroy_process_group()


def flush_c_stdio():
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: the other BASELINE configs, roofline legs, the CPU baseline, "
                         "the auxiliary forwards, and the headline as the median of --repeats windows (default: the headline alone, "
                         "one window of --steps steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step's convert() returned to DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--headline-only", action="store_true", help="skip the lines of the other BASELINE configs")
    ap.add_argument("--jobs", type=int, default=4,
                    help="convert() calls in flight per GPU, each on its own HIP stream (the reference's "
                         "jobs_per_compute_device, satools/satools/bin/anonymize:85-93)")
    ap.add_argument("--gather", choices=("f32", "pcm16"), default="f32",
                    help="sharded mode: gather the waveforms as f32 (default) or as the int16 PCM the reference writes (half the bytes)")
    ap.add_argument("--repeats", type=int, default=None,
                    help="timed windows of --steps steps each; `value` = the median window (SURVEY 8(d): median of >= 5 repeats); "
                         "default 5 with --full, else 1")
    ap.add_argument("--gather-chunk", type=int, default=4,
                    help="sharded mode: the waveform exchange is issued in chunks of this many batches on a communication stream while "
                         "the shard is still being computed (0 = one all_gather_into_tensor at the end)")
    ap.add_argument("--f0-status", choices=("sync", "deferred"), default="deferred",
                    help="when a batch's deferred work (YAAPT's status word, the near-tie utterances of the VQ) is checked: before the same job's "
                         "next batch (default: convert(..., defer_status=True), what the batch job does) or inside every convert() call (the plain "
                         "call: the one launching thread then waits for the GPU in every step; measured beside the headline as "
                         "`configs[\"configs[1] plain convert()\"]`)")
    ap.add_argument("--gen-precision", default=None,
                    help="generator arithmetic of every line (default: the package default, SATOOLS_AMD_GEN_PRECISION); when that is "
                         "f16f8r the headline tag is also measured as f16x3 and kept in `configs`")
    ap.add_argument("--cpu-worker", nargs=4, metavar=("TAG", "F0TR", "N", "INDEX"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-config", default=None, help=argparse.SUPPRESS)       # JSON spec of ONE side config measured in its own process
    ap.add_argument("--tag", default=None, help="measure only this tag (one line)")
    ap.add_argument("--f0-transformation", default="", help="with --tag: e.g. quant_16_awgn_2")
    a = ap.parse_args()
    a.jobs = max(1, a.jobs)
    a.repeats = max(1, a.repeats if a.repeats is not None else (5 if a.full else 1))
    if a.cpu_worker:
        return cpu_worker(a.cpu_worker[0], a.cpu_worker[1], int(a.cpu_worker[2]), int(a.cpu_worker[3]))

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # typed as `python bench.py --gpus N`: start the ranks as a CHILD process (this parent has not touched the GPU
        # and never does — no exec of a process that initialised HIP) and relay its output and exit code
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, MASTER_ADDR="127.0.0.1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.exit(subprocess.call(cmd, env=env))

    # N = 1, --full run: every config but the headline is measured in its OWN process, one after the other, BEFORE this process touches
    # the GPU (round 6: in one process the later configs of a run were slower than the same config alone — per-step host waits with a
    # heavier tail, and a device-wide slowdown for the rest of the process once a high-priority stream had been created, DESIGN toolchain
    # note 22 — so a line must not depend on what ran before it).  The children print their full line; the headline runs here, last.
    child_lines = []
    side_in_children = (a.full and a.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and not a.tag and not a.headline_only and not a.child_config and
                        os.environ.get("SAT_BENCH_FORCE_PG") != "1" and os.environ.get("SAT_BENCH_DRYRUN") != "1")
    if side_in_children:
        k2 = min(a.steps, 12)
        specs = [dict(name="configs[2]", tag=TAG_W2V2, f0_tr="", steps=k2, warmup=a.warmup,
                      cpu_args=dict(n_utt=8, runs_1=1, runs_n=3, n_utt_1=4, procs=8, n_utt_proc=2)),
                 dict(name="configs[3]", tag=TAG_W2V2, f0_tr="quant_16_awgn_2", steps=k2, warmup=a.warmup,
                      cpu_args=dict(n_utt=8, runs_1=1, runs_n=1, n_utt_1=2,
                                    budget_note="; configs[3] differs from configs[2] by the quantisation + noise of 250 x B values only, so its CPU leg is a shorter sample"))]
        prec0 = a.gen_precision or os.environ.get("SATOOLS_AMD_GEN_PRECISION", "f16f8r")
        if prec0 == "f16f8r":
            # the headline tag on the f16x3 generator too, beside the headline (same run, same box)
            specs.append(dict(name="configs[1] generator f16x3", tag=TAG, f0_tr="", steps=a.steps, warmup=a.warmup, cpu_args=None, gen_precision="f16x3"))
        if a.f0_status == "deferred":
            # ... and with the plain convert() call (rounds 1-5 measured the headline that way)
            specs.append(dict(name="configs[1] plain convert()", tag=TAG, f0_tr="", steps=a.steps, warmup=a.warmup, cpu_args=None, status="sync", roofline=False))
        if BATCH == 32:
            # ... and at twice the batch (NOT the configuration the metric is quoted on: the size of a batch is the batch job's choice, and the
            # latency-bound extractor launches serve 64 utterances in the time of 32)
            specs.append(dict(name="configs[1] at batch 64 (not the quoted configuration)", tag=TAG, f0_tr="", steps=max(a.steps // 2, 4), warmup=a.warmup,
                              cpu_args=None, roofline=False, env={"SAT_BENCH_BATCH": "64"}))
        for spec in specs:
            spec["repeats"] = min(a.repeats, 3)
            child_env = dict(os.environ, **spec.pop("env", {}))
            cmd = [sys.executable, os.path.abspath(__file__), "--full", "--child-config", json.dumps(spec), "--jobs", str(a.jobs), "--f0-status", a.f0_status,
                   "--gather", a.gather] + (["--no-cpu-baseline"] if a.no_cpu_baseline else []) + (["--gen-precision", a.gen_precision] if a.gen_precision else [])
            # (a side config that fails or hangs must not take the headline with it: it is reported on stderr and left out of `configs`)
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900, env=child_env)
                got = [l for l in r.stdout.splitlines() if l.startswith("{")]
                if r.returncode != 0 or not got:
                    raise RuntimeError(f"exit code {r.returncode}")
                child_lines.append(json.loads(got[-1]))
            except Exception as e:      # noqa: BLE001
                print(f"bench.py: the child process measuring {spec['name']} failed ({e!r}): that config is missing from this line", file=sys.stderr, flush=True)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("SAT_BENCH_DRYRUN") == "1":
        return dryrun(a, rank, world)
    if a.gpus != world and not (a.gpus == 1 and world == 1):
        print(f"bench.py --gpus {a.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # SAT_BENCH_FORCE_PG=1: take the sharded RCCL path with one rank too (checked on a 1-GPU box)
    use_pg = world > 1 or os.environ.get("SAT_BENCH_FORCE_PG") == "1"
    if use_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)
        # RCCL writes a version banner to the C stdout of rank 0, which leaves its buffer only at exit — AFTER the JSON
        # line unless it is flushed now: build the communicator with one small collective, then flush C stdio
        t = torch.zeros(1, device=dev)
        dist.all_reduce(t)
        torch.cuda.synchronize()
        flush_c_stdio()

    want_cpu = a.full and (not a.no_cpu_baseline) and world == 1 and not use_pg
    lines = list(child_lines)
    if a.child_config:
        # one side config, alone in this process: its full line on stdout
        spec = json.loads(a.child_config)
        cpu_args = spec.get("cpu_args")
        out = one_config(spec["name"], spec["tag"], spec["f0_tr"], a, dev, rank, world, False, spec["steps"], spec["warmup"],
                         want_cpu and cpu_args is not None, cpu_args or {}, repeats=spec.get("repeats", 3),
                         gen_precision=spec.get("gen_precision") or a.gen_precision, status=spec.get("status"), want_roofline=spec.get("roofline", True))
        print(json.dumps(out), flush=True)
        return
    if a.tag:
        plan = [("--tag", a.tag, a.f0_transformation, a.steps, a.warmup, dict(n_utt=8, runs_1=1, runs_n=3, n_utt_1=4))]
    elif use_pg:
        k2 = min(a.steps, 16)
        plan = ([] if a.headline_only or not a.full else [("configs[4]", TAG_W2V2, "", k2, min(a.warmup, 4), None)]) + \
               [("configs[1] sharded", TAG, "", a.steps, a.warmup, None)]
    else:
        # (the other configs of a default N = 1 run were measured in child processes above)
        plan = [("configs[1]", TAG, "", a.steps, a.warmup, dict(n_utt=8, runs_1=3, runs_n=3, procs=32, n_utt_proc=4))]
    for i, (name, tag, f0_tr, steps, warmup, cpu_args) in enumerate(plan):
        headline = i == len(plan) - 1
        out = one_config(name, tag, f0_tr, a, dev, rank, world, use_pg, steps, warmup, want_cpu and cpu_args is not None, cpu_args or {},
                         repeats=a.repeats if headline else min(a.repeats, 3), gen_precision=a.gen_precision, want_roofline=a.full,
                         dump=a.dump_outputs if headline else None)
        torch.cuda.empty_cache()
        if rank == 0:
            lines.append(out)
    if rank == 0:
        # the contract is ONE JSON line on stdout: the headline.  The full lines of the other configs go to stderr
        # (prefixed CONFIG_LINE) and, condensed, into the headline's `configs` object
        head = lines[-1]
        if len(lines) > 1:
            def brief(o):
                r, c = o.get("roofline"), o["config"]
                d = {"workload": c["workload"].split(" model.convert")[0], "value": o["value"], "unit": "x real-time", "ms_per_step": o["ms_per_step"],
                     "steps": o["steps"], "n_gpus": o["n_gpus"], "windows": o["repeats"]["windows"], "value_min_max": o["repeats"]["value_min_max"],
                     "generator_precision": c["generator_precision"], "dtype": o["dtype"], "f0_status": c["f0_status"].split(":")[0].split(",")[0],
                     "vq_near_tie_guard": c.get("vq_near_tie_guard")}
                if r is not None:
                    d["roofline"] = {"bound": r["bound"], "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"],
                                     "kernel": r["kernel"].split(":")[0],
                                     "dominant_kernel_frac": (r.get("dominant_kernel") or {}).get("frac")}
                for k in ("all_gather_ms", "ranks_seen_by_rccl", "utterances"):
                    if k in c:
                        d[k] = c[k]
                if "cpu_baseline" in o:
                    cb = o["cpu_baseline"]
                    d["cpu_baseline"] = {"value": cb["value"], "cores": cb["cores"], "threads1": cb["threads1"]["value"],
                                         "threadsN": cb["threadsN"]["value"], "threadsN_cores": cb["threadsN"]["threads"], "kind": cb["kind"]}
                    if "processes" in cb:
                        d["cpu_baseline"]["processes"] = {"value": cb["processes"]["value"], "processes": cb["processes"]["processes"]}
                return d
            head["configs"] = {o["config"]["workload"].split(":")[0]: brief(o) for o in lines[:-1]}
            if not use_pg and not a.tag and side_in_children:
                head["configs"].update(aux_forwards(dev))
            for o in lines[:-1]:
                print("CONFIG_LINE " + json.dumps(o), file=sys.stderr, flush=True)
    if use_pg:
        dist.barrier()
        dist.destroy_process_group()
    flush_c_stdio()            # whatever native libraries buffered on stdout comes out BEFORE the line
    if rank == 0:
        print(json.dumps(lines[-1]), flush=True)       # the ONE JSON line, last on stdout


if __name__ == "__main__":
    main()
