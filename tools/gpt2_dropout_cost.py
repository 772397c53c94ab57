#!/usr/bin/env python3
"""Cost of dropout on the GPT-2 training step: the whole step (forward, loss, backward, grad-norm clip,
capturable AdamW) captured once into a hipGraph per arm and replayed -- once with every probability
at 0.0 (the step bench.py measures) and once with embd / attn / resid dropout at --p.  Every replay is
timed with its own event pair; arms are interleaved round by round; one JSON line with the median.

    python tools/gpt2_dropout_cost.py [--batch-size 16] [--seq-len 1024] [--layers 12] [--p 0.1]
                                      [--replays 20] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_distributed_example_amd.data import synthetic_tokens  # noqa: E402
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2  # noqa: E402
from pytorch_distributed_example_amd.optim import AdamWMaster  # noqa: E402


def build_arm(p, a, dev, tokens):
    cfg = GPTConfig(block_size=max(1024, a.seq_len), n_layer=a.layers, embd_pdrop=p, attn_pdrop=p, resid_pdrop=p)
    model = build_gpt2(cfg, seed=0, device=dev).seed_dropout(1234)
    opt = AdamWMaster(model.decay_groups(0.1), lr=6e-4, betas=(0.9, 0.95), max_grad_norm=1.0, capturable=True)
    sx, sy = tokens[:, :-1].contiguous(), tokens[:, 1:].contiguous()
    ones = torch.ones((), device=dev, dtype=torch.float32)

    def step():
        opt.zero_grad()
        loss = model(sx, sy)
        loss.backward(ones)
        opt.step()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    graph.replay()                      # first launch outside the timed rounds
    torch.cuda.synchronize()
    # the graph holds raw addresses of everything the step touched: the optimizer state and the static
    # inputs must outlive it (the next arm's capture empties the allocator cache, which would unmap them)
    return {"graph": graph, "loss": loss, "model": model, "keep": (opt, sx, sy, ones, step)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    tokens = synthetic_tokens(torch.arange(a.batch_size), a.seq_len, GPTConfig().vocab_size, seed=0, device=dev)
    arms = {"p0": build_arm(0.0, a, dev, tokens), "dropout": build_arm(a.p, a, dev, tokens)}
    times = {k: [] for k in arms}
    for r in range(a.rounds + 1):                        # round 0 is warm-up
        for name, arm in arms.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(a.replays)]
            torch.cuda.synchronize()
            for s, e in ev:
                s.record()
                arm["graph"].replay()
                e.record()
            torch.cuda.synchronize()
            if r:
                times[name] += [round(s.elapsed_time(e), 4) for s, e in ev]
    med = {k: statistics.median(v) for k, v in times.items()}
    rng = arms["dropout"]["model"].rng
    print(json.dumps({
        "metric": "gpt2_step_ms_graph_replay", "batch_size": a.batch_size, "seq_len": a.seq_len, "layers": a.layers,
        "p": a.p, "replays_per_arm": len(times["p0"]), "median_ms": med,
        "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
        "dropout_cost_ms": round(med["dropout"] - med["p0"], 4),
        "dropout_cost_pct": round(100.0 * (med["dropout"] / med["p0"] - 1.0), 2),
        "last_loss": {k: float(v["loss"]) for k, v in arms.items()},
        "rng_draws": rng.draw_number(), "p0_rng_created": arms["p0"]["model"]._rng is not None}))


if __name__ == "__main__":
    main()
