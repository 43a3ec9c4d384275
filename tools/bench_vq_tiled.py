"""Kernel time of the tiled VQ kernel (csrc/vq_tiled.hip) at the 256-code tag's shape — B = 32, D = 256, T = 250, 256 codes, with and
without the near-tie count — beside the LDS-resident kernel (csrc/bottleneck.hip) at 64 codes on the same z, alternated in one
call.  The 256-code launch does four times the arithmetic and stages four times the codebook: 4 x the 64-code launch is the figure
to compare with.  Before timing: the two kernels' bits at 64 codes are compared (dist, idx, q, tie_count).
    python tools/bench_vq_tiled.py [--rounds 5] [--launches 200]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import satools_amd  # noqa: E402,F401
from satools_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=200)
a = ap.parse_args()
dev = "cuda"
B, D, T = 32, 256, 250
g = torch.Generator().manual_seed(0)
z = torch.randn(B, D, T, generator=g)
frames = z.permute(0, 2, 1).reshape(-1, D)
cb256 = (frames[torch.randperm(B * T, generator=g)[:256]] + 0.3 * torch.randn(256, D, generator=g)).contiguous()
z, cb256 = z.to(dev), cb256.to(dev)
cb64 = cb256[:64].contiguous()
pair = lambda cb: torch.cdist(cb.double(), cb.double()).float().contiguous()
p64, p256 = pair(cb64), pair(cb256)
counts = lambda: torch.tensor([[0] * B, [2 ** 31 - 1] * B, [-1] * B], dtype=torch.int32, device=dev)
SCALE = 1e-3

# the twin check: same bits at 64 codes
c0, c1 = counts(), counts()
r0 = ops.vq(z, cb64, want_dist=True, tie=(p64, SCALE, c0))
r1 = ops.vq_tiled(z, cb64, want_dist=True, tie=(p64, SCALE, c1))
torch.cuda.synchronize()
same = all(torch.equal(x, y) for x, y in zip(r0, r1)) and torch.equal(c0, c1)
print(f"64 codes, tiled vs LDS-resident kernel: bits equal = {same} ({int(c0[0].sum())} near-tie frames counted by both)")
if not same:
    sys.exit("the two kernels differ at 64 codes")

cnt = counts()
legs = {
    "lds 64": lambda: ops.vq(z, cb64),
    "lds 64 tie": lambda: ops.vq(z, cb64, tie=(p64, SCALE, cnt)),
    "tiled 64": lambda: ops.vq_tiled(z, cb64),
    "tiled 256": lambda: ops.vq_tiled(z, cb256),
    "tiled 256 tie": lambda: ops.vq_tiled(z, cb256, tie=(p256, SCALE, cnt)),
}


def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for f in legs.values():
    timed(f, 20)
res = {k: [] for k in legs}
for _ in range(a.rounds):                      # alternated: every leg once per round
    for k, f in legs.items():
        res[k].append(timed(f, a.launches))
med = {k: statistics.median(v) for k, v in res.items()}
for k, v in res.items():
    print(f"{k:14s}: median {med[k]:7.1f} us per launch (min {min(v):.1f}, max {max(v):.1f}; {a.rounds} x {a.launches} launches, device events)")
print(f"tiled 256 / lds 64 = {med['tiled 256'] / med['lds 64']:.2f} (4 = the same time per code); "
      f"with the near-tie count {med['tiled 256 tie'] / med['lds 64 tie']:.2f}; tiled 64 / lds 64 = {med['tiled 64'] / med['lds 64']:.2f}")
