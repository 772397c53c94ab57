#!/usr/bin/env python3
"""Cost of the smoothed and weighted loss (the SMOOTH softmax-CE kernels), graph-replayed medians.

(a) kernels, at N = 16384 rows of the GPT-2 vocabulary (V = 50257, Vp = 50304): the MASK call with nothing
    ignored (the baseline) against the SMOOTH call with label smoothing alone, z-loss alone, weights alone and
    all three.  Every case is captured as one hipGraph of ``--calls`` calls on the same buffers (the CE call
    rewrites the logits in place, so from its second call on it reads gradients: the kernels have no
    data-dependent path but the ignored-row exit, which depends on the targets only); a figure is the median
    over the replays of replay time / calls, the cases alternating inside every round.
(b) the GPT-2 training step (forward, loss, backward, grad-norm clip, capturable AdamW) captured once per arm:
    the plain step, and the step with ``label_smoothing``, ``z_loss`` and ``loss_weights`` all on.

One JSON line per case.  Each part is one process; run each under its own time limit:

    timeout -k 10 300 python tools/loss_smoothing_bench.py --part a [--rows 16384] [--calls 10] [--replays 20]
    timeout -k 10 300 python tools/loss_smoothing_bench.py --part b [--batch-size 16] [--seq-len 1024] [--layers 12]
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
from pytorch_distributed_example_amd import ops  # noqa: E402
from pytorch_distributed_example_amd._ext import kernels  # noqa: E402
from pytorch_distributed_example_amd.data import synthetic_tokens  # noqa: E402
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2  # noqa: E402
from pytorch_distributed_example_amd.optim import AdamWMaster  # noqa: E402

EPS, ZC = 0.1, 1e-4


def part_a(a, dev):
    K = kernels()
    N, V, Vp = a.rows, 50257, 50304
    g = torch.Generator().manual_seed(0)
    logits = torch.empty(N, Vp, device=dev, dtype=torch.bfloat16).normal_(0.0, 3.0)
    rows = torch.empty(N, device=dev)
    lt = ops.loss_targets(torch.randint(0, V, (N,), generator=g).to(dev), vocab_size=V)
    wt = (2 * torch.rand(N, generator=g)).to(dev)

    def ce(**kw):
        return lambda: K.xent_bf16(logits, lt.targets, V, 1.0, rows, True, scale_dev=lt.inv, **kw)

    cases = {
        "xent_mask": ce(), "xent_eps": ce(label_smoothing=EPS), "xent_zc": ce(z_loss=ZC),
        "xent_weights": ce(loss_weights=wt), "xent_all": ce(label_smoothing=EPS, z_loss=ZC, loss_weights=wt),
    }

    def many(fn):
        def run():
            for _ in range(a.calls):
                fn()
        return run

    graphs = {}
    for name, fn in cases.items():
        graphs[name], _ = capture(many(fn))
    times = replay_rounds(graphs, a.replays, a.rounds)
    med = {}
    for name, v in times.items():
        per = [t / a.calls * 1e3 for t in v]
        med[name] = statistics.median(per)
        print(json.dumps({"part": "a", "case": name, "rows": N, "V": V, "Vp": Vp, "us_per_call": round(med[name], 2),
                          "us_min_max": [round(min(per), 2), round(max(per), 2)], "calls_per_graph": a.calls,
                          "replays": len(per)}), flush=True)
    print(json.dumps({"part": "a", "smooth_over_mask": {k: round(med[k] / med["xent_mask"], 4)
                                                         for k in med if k != "xent_mask"}}), flush=True)


def build_arm(smooth, a, dev, tokens):
    cfg = GPTConfig(block_size=max(1024, a.seq_len), n_layer=a.layers)
    model = build_gpt2(cfg, seed=0, device=dev)
    opt = AdamWMaster(model.decay_groups(0.1), lr=6e-4, betas=(0.9, 0.95), max_grad_norm=1.0, capturable=True)
    sx, sy = tokens[:, :-1].contiguous(), tokens[:, 1:].contiguous()
    kw = {}
    if smooth:
        wt = (2 * torch.rand(sy.shape, generator=torch.Generator().manual_seed(1))).to(dev)
        kw = dict(label_smoothing=EPS, z_loss=ZC, loss_weights=wt)
    ones = torch.ones((), device=dev, dtype=torch.float32)

    def step():
        opt.zero_grad()
        loss = model(sx, sy, **kw)
        loss.backward(ones)
        opt.step()
        return loss.detach()

    graph, loss = capture(step)
    # the graph holds raw addresses of everything the step touched: keep it all alive
    return {"graph": graph, "loss": loss, "keep": (model, opt, sx, sy, ones, step, kw)}


def part_b(a, dev):
    tokens = synthetic_tokens(torch.arange(a.batch_size), a.seq_len, GPTConfig().vocab_size, seed=0, device=dev)
    arms = {"plain": build_arm(False, a, dev, tokens), "smooth_all": build_arm(True, a, dev, tokens)}
    times = replay_rounds({k: v["graph"] for k, v in arms.items()}, a.replays, a.rounds)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(json.dumps({"part": "b", "case": k, "metric": "gpt2_step_ms_graph_replay", "batch_size": a.batch_size,
                          "seq_len": a.seq_len, "layers": a.layers, "median_ms": round(med[k], 4),
                          "min_max_ms": [round(min(v), 4), round(max(v), 4)], "replays": len(v),
                          "vs_plain_pct": round(100.0 * (med[k] / med["plain"] - 1.0), 2),
                          "last_loss": float(arms[k]["loss"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"], required=True)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_smoothing_bench: needs a GPU (no CPU timing exists)")
    dev = torch.device("cuda", 0)
    {"a": part_a, "b": part_b}[a.part](a, dev)


if __name__ == "__main__":
    main()
