#!/usr/bin/env python3
"""Cost of a learning-rate table on the toy-CNN step: the same engine, the same graph-replayed steps,
once with the by-value rate and once with a warm-up + cosine table attached (the optimizer kernel's
extra block-uniform read).  Arms are interleaved; one JSON line with every timing and the medians.

    python tools/lr_schedule_bench.py [--steps 2000] [--graph-steps 10] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_distributed_example_amd.data import synthetic_mnist  # noqa: E402
from pytorch_distributed_example_amd.engine import LeNetTrainStep  # noqa: E402
from pytorch_distributed_example_amd.models import build_net  # noqa: E402
from pytorch_distributed_example_amd.optim import lr_scheduler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--graph-steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=128)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ds = synthetic_mnist(60000, seed=0, device=dev)
    idx = torch.randperm(len(ds.labels), generator=torch.Generator().manual_seed(0)).to(torch.int32)
    idx = idx[: idx.numel() // a.batch_size * a.batch_size]       # full batches only: every step is B


    engines = {}
    for arm in ("by_value", "table"):
        sched = lr_scheduler.warmup_cosine(1e-3, 100, a.steps * (a.repeats + 1)) if arm == "table" else None
        eng = LeNetTrainStep(build_net(seed=0, device=dev), batch_size=a.batch_size, lr_schedule=sched)
        eng.bind_dataset(ds.images, ds.labels)
        eng.set_epoch_indices(idx)
        eng.prime_graphs((a.graph_steps,))
        engines[arm] = eng
    reps = a.steps // a.graph_steps
    times = {arm: [] for arm in engines}
    for r in range(a.repeats + 1):                       # round 0 is warm-up
        for arm, eng in engines.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(reps):
                eng.replay(steps=a.graph_steps)
            e.record()
            torch.cuda.synchronize()
            if r:
                times[arm].append(round(s.elapsed_time(e) / (reps * a.graph_steps), 5))
    print(json.dumps({"metric": "lenet_ms_per_step", "steps": reps * a.graph_steps, "graph_steps": a.graph_steps,
                      "ms_per_step": times, "median": {k: statistics.median(v) for k, v in times.items()},
                      "table_lr_next": engines["table"].current_lr()}))


if __name__ == "__main__":
    main()
