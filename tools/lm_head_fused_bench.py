#!/usr/bin/env python3
"""No-gradient LM-head loss with and without the logits buffer, graph-replayed medians and peak memory.

At C = 768, V = 50257, Vp = 50304 and every ``--rows`` value: ``lm_head_loss(reduction="none")`` under
``torch.no_grad()`` as it is (``gemm.fprop`` with ``nt_out`` writes [N, Vp] bf16 logits, loss-only ``xent_bf16``
reads them back) against ``fused=True`` (``lm_head_stats``' kernels).  Each arm is captured as one hipGraph of
``--calls`` calls; a figure is the median over the replays of replay time / calls, the arms alternating inside every
round, with min and max as the spread.  Peak memory is ``torch.cuda.max_memory_allocated`` over one eager call of
each arm, above what was allocated before it; the fused arm must save at least ``N * Vp * 2`` bytes less its
partials ``S * N * 16``.  The arms' rows are compared too.  One JSON line per arm and size.

    timeout -k 10 300 python tools/lm_head_fused_bench.py [--rows 16384 1024] [--calls 5] [--replays 10] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from masked_loss_bench import capture, replay_rounds  # noqa: E402
from pytorch_distributed_example_amd._ext import kernels  # noqa: E402
from pytorch_distributed_example_amd.ops import transformer as TR  # noqa: E402

C, V, VP = 768, 50257, 50304


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def bench(N, a, dev):
    g = torch.Generator().manual_seed(0)
    h = torch.randn(N, C, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(VP, C, generator=g) * 0.05).to(dev, torch.bfloat16)
    tg = torch.randint(0, V, (N,), generator=g).to(dev)
    arms = {"logits": lambda: TR.lm_head_loss(h, w, tg, V, ignore_index=-1, reduction="none"),
            "fused": lambda: TR.lm_head_loss(h, w, tg, V, ignore_index=-1, reduction="none", fused=True)}

    def many(fn):
        def run():
            for _ in range(a.calls):
                out = fn()
            return out
        return run

    with torch.no_grad():
        for fn in arms.values():    # first calls: code objects, the allocator's pools
            fn()
        peaks, outs = {}, {}
        for name, fn in arms.items():
            peaks[name], outs[name] = peak_bytes(fn)
        diff = (outs["fused"] - outs["logits"]).abs().max().item()
        del outs
        torch.cuda.empty_cache()
        graphs = {name: capture(many(fn))[0] for name, fn in arms.items()}
        times = replay_rounds(graphs, a.replays, a.rounds)
    S = kernels().lm_head_slices(N, V)
    need = N * VP * 2 - S * N * 16
    med = {k: statistics.median(t / a.calls for t in v) for k, v in times.items()}
    for name, v in times.items():
        per = [t / a.calls for t in v]
        print(json.dumps({"case": name, "rows": N, "C": C, "V": V, "Vp": VP, "ms_per_call": round(med[name], 4),
                          "ms_min_max": [round(min(per), 4), round(max(per), 4)], "calls_per_graph": a.calls,
                          "replays": len(per), "peak_bytes": peaks[name]}), flush=True)
    print(json.dumps({"rows": N, "slices": S, "fused_over_logits": round(med["fused"] / med["logits"], 4),
                      "peak_saved_bytes": peaks["logits"] - peaks["fused"], "peak_saved_required": need,
                      "peak_ok": peaks["logits"] - peaks["fused"] >= need, "max_row_diff": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[16384, 1024])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lm_head_fused_bench: needs a GPU (no CPU timing exists)")
    dev = torch.device("cuda", 0)
    for N in a.rows:
        bench(N, a, dev)


if __name__ == "__main__":
    main()
