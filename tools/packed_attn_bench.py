#!/usr/bin/env python3
"""Document-masked flash attention (the DOC instantiations of csrc/kernels/attention.hip) at the GPT-2 small
shape (B=16, T=1024, H=12, D=64) against the plain causal kernels: forward and backward time per call for

  plain     the kernels without documents
  doc_one   DOC with one document per row: the price of the extra mask and the bounds loads
  doc_256   DOC with seeded random documents of mean length 256: what the skipped tiles save

Event-timed; the cases alternate inside every repeat and the figure of a case is the median over the repeats.
One JSON line per case, then one with the ratios.

usage: python tools/packed_attn_bench.py [--iters 200] [--reps 9] [--mean-len 256]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd._ext import kernels


def random_doc_ids(B, T, mean_len, seed):
    """[B, T] ids: every position after the first starts a new document with probability 1 / mean_len."""
    g = torch.Generator().manual_seed(seed)
    starts = torch.rand(B, T, generator=g) < 1.0 / mean_len
    starts[:, 0] = True
    return starts.cumsum(1)


def visible_pairs(doc_start):
    """Number of (query, key) pairs the mask admits: sum over t of t - doc_start[t] + 1."""
    T = doc_start.shape[1]
    return int((torch.arange(T, device=doc_start.device)[None, :] - doc_start + 1).sum().item())


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--mean-len", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("packed_attn_bench: needs a GPU (no CPU timing exists)")
    K = kernels()
    B, T, H, D = a.B, a.T, a.H, 64
    C = H * D
    torch.manual_seed(a.seed)
    qkv = torch.randn(B, T, 3 * C, device="cuda").to(torch.bfloat16)
    q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    o = torch.empty(B, T, C, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B * H * T, device="cuda")
    do = torch.randn(B, T, C, device="cuda").to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:]
    Dd = torch.empty(B * H * T, device="cuda")
    scale = 1.0 / math.sqrt(D)
    one = ops.doc_bounds(torch.zeros(B, T, dtype=torch.int64, device="cuda"))
    packed = ops.doc_bounds(random_doc_ids(B, T, a.mean_len, a.seed).cuda())
    nodrop = (None, 0, 0, 1.0)
    cases = {"plain": None, "doc_one": one, f"doc_{a.mean_len}": packed}

    def fwd(bounds):
        if bounds is None:
            return lambda: K.attn_fwd(q, k, v, o, lse, H, scale)
        return lambda: K.attn_fwd(q, k, v, o, lse, H, scale, *nodrop, bounds[0])

    def bwd(bounds):
        if bounds is None:
            return lambda: K.attn_bwd(q, k, v, o, do, lse, Dd, dq, dk, dv, H, scale)
        return lambda: K.attn_bwd(q, k, v, o, do, lse, Dd, dq, dk, dv, H, scale, *nodrop, *bounds)

    times = {n: {"fwd": [], "bwd": []} for n in cases}
    for n, bnd in cases.items():            # warm-up of every case: code objects, clocks
        for _ in range(3):
            fwd(bnd)()                      # the backward of a case reads the o and lse of its own forward
            bwd(bnd)()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for n, bnd in cases.items():
            fwd(bnd)()
            times[n]["fwd"].append(timed(fwd(bnd), a.iters))
            times[n]["bwd"].append(timed(bwd(bnd), a.iters))
    med = {}
    full = B * T * (T + 1) // 2
    for n, bnd in cases.items():
        pairs = full if bnd is None else visible_pairs(bnd[0])
        med[n] = {p: statistics.median(times[n][p]) for p in ("fwd", "bwd")}
        print(json.dumps({"case": n, "shape": [B, T, H, D], "visible_pairs_vs_causal": round(pairs / full, 4),
                          "fwd_us": round(med[n]["fwd"], 1), "bwd_us": round(med[n]["bwd"], 1),
                          "fwd_us_min_max": [round(min(times[n]["fwd"]), 1), round(max(times[n]["fwd"]), 1)],
                          "bwd_us_min_max": [round(min(times[n]["bwd"]), 1), round(max(times[n]["bwd"]), 1)],
                          "iters": a.iters, "reps": a.reps}), flush=True)
    pk = f"doc_{a.mean_len}"
    print(json.dumps({"doc_one_over_plain": {p: round(med["doc_one"][p] / med["plain"][p], 4) for p in ("fwd", "bwd")},
                      "plain_over_packed": {p: round(med["plain"][p] / med[pk][p], 3) for p in ("fwd", "bwd")}}),
          flush=True)


if __name__ == "__main__":
    main()
