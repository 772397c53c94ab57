#!/usr/bin/env python3
"""Cost of the masked loss (ops.loss_targets, the MASK softmax-CE kernels), graph-replayed medians.

(a) kernels, at N = 16384 rows of the GPT-2 vocabulary (V = 50257, Vp = 50304): the unmasked fused
    softmax-CE call against the MASK call with 0 %, 50 % and 90 % of the rows ignored, ``k_loss_targets``
    alone, and -- for scale -- the three LM-head GEMMs (logits, dh, dW) that a masked row still pays for.
    Every case is captured as one hipGraph of ``--calls`` calls on the same buffers (the CE call rewrites the
    logits in place, so from its second call on it reads gradients: the kernels have no data-dependent path
    but the ignored-row exit, which depends on the targets only); a figure is the median over the replays
    of replay time / calls, the cases alternating inside every round.
(b) the GPT-2 training step (forward, loss, backward, grad-norm clip, capturable AdamW) captured once per
    arm: the plain step, and the step with ``ignore_index=-100`` at 0 % and 50 % of the targets ignored.

One JSON line per case.

    python tools/masked_loss_bench.py [--part a|b|ab] [--rows 16384] [--calls 10] [--replays 20] [--rounds 3]
                                      [--batch-size 16] [--seq-len 1024] [--layers 12]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_distributed_example_amd import ops  # noqa: E402
from pytorch_distributed_example_amd._ext import kernels  # noqa: E402
from pytorch_distributed_example_amd.data import synthetic_tokens  # noqa: E402
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2  # noqa: E402
from pytorch_distributed_example_amd.ops import gemm as G  # noqa: E402
from pytorch_distributed_example_amd.optim import AdamWMaster  # noqa: E402


def capture(fn, warm=2):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    graph.replay()                          # first launch outside the timed rounds
    torch.cuda.synchronize()
    return graph, out


def replay_rounds(graphs, replays, rounds):
    """ms per replay of every graph: every replay under its own event pair, graphs alternating per round,
    round 0 thrown away."""
    times = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for name, graph in graphs.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(replays)]
            torch.cuda.synchronize()
            for s, e in ev:
                s.record()
                graph.replay()
                e.record()
            torch.cuda.synchronize()
            if r:
                times[name] += [s.elapsed_time(e) for s, e in ev]
    return times


def part_a(a, dev):
    K = kernels()
    N, V, Vp, C = a.rows, 50257, 50304, 768
    g = torch.Generator().manual_seed(0)
    logits = torch.empty(N, Vp, device=dev, dtype=torch.bfloat16).normal_(0.0, 3.0)
    rows = torch.empty(N, device=dev)
    tg = torch.randint(0, V, (N,), generator=g)
    keep = []

    def ce(frac):
        if frac is None:
            t = tg.to(dev)
            keep.append(t)
            return lambda: K.xent_bf16(logits, t, V, 1.0 / N, rows, True)
        lt = ops.loss_targets(tg.masked_fill(torch.rand(N, generator=g) < frac, -100).to(dev), vocab_size=V,
                              ignore_index=-100)
        keep.append(lt)
        return lambda: K.xent_bf16(logits, lt.targets, V, 1.0, rows, True, scale_dev=lt.inv)

    raw = tg.masked_fill(torch.rand(N, generator=g) < 0.5, -100).to(dev)
    mask = (torch.rand(N, generator=g) < 0.5).to(dev)
    h = torch.randn(N, C, device=dev).to(torch.bfloat16)
    w = (0.02 * torch.randn(Vp, C, device=dev)).to(torch.bfloat16)
    one = torch.ones(1, device=dev)
    out = torch.empty_like(logits)
    cases = {
        "xent_unmasked": ce(None), "xent_mask_0pct": ce(0.0), "xent_mask_50pct": ce(0.5), "xent_mask_90pct": ce(0.9),
        "loss_targets": lambda: ops.loss_targets(raw, vocab_size=V, ignore_index=-100, loss_mask=mask),
        "lm_head_fprop": lambda: G.fprop(h, w, out=out, nt_out=True),
        "lm_head_dgrad": lambda: G.dgrad(logits, w, scale=one),
        "lm_head_wgrad": lambda: G.wgrad(logits, h, scale=one),
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
    print(json.dumps({"part": "a", "mask_over_unmasked": {k: round(med[k] / med["xent_unmasked"], 4)
                                                           for k in med if k.startswith("xent_mask")},
                      "lm_head_gemms_us": round(sum(med[k] for k in med if k.startswith("lm_head")), 1)}), flush=True)


def build_arm(frac, a, dev, tokens):
    cfg = GPTConfig(block_size=max(1024, a.seq_len), n_layer=a.layers)
    model = build_gpt2(cfg, seed=0, device=dev)
    opt = AdamWMaster(model.decay_groups(0.1), lr=6e-4, betas=(0.9, 0.95), max_grad_norm=1.0, capturable=True)
    sx, sy = tokens[:, :-1].contiguous(), tokens[:, 1:].contiguous()
    kw = {}
    if frac is not None:
        drop = torch.rand(sy.shape, generator=torch.Generator().manual_seed(1)) < frac
        sy = sy.masked_fill(drop.to(dev), -100)
        kw = dict(ignore_index=-100)
    ones = torch.ones((), device=dev, dtype=torch.float32)

    def step():
        opt.zero_grad()
        loss = model(sx, sy, **kw)
        loss.backward(ones)
        opt.step()
        return loss.detach()

    graph, loss = capture(step)
    # the graph holds raw addresses of everything the step touched: keep it all alive
    return {"graph": graph, "loss": loss, "keep": (model, opt, sx, sy, ones, step)}


def part_b(a, dev):
    tokens = synthetic_tokens(torch.arange(a.batch_size), a.seq_len, GPTConfig().vocab_size, seed=0, device=dev)
    arms = {"plain": build_arm(None, a, dev, tokens), "ignore_0pct": build_arm(0.0, a, dev, tokens),
            "ignore_50pct": build_arm(0.5, a, dev, tokens)}
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
    ap.add_argument("--part", choices=["a", "b", "ab"], default="ab")
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("masked_loss_bench: needs a GPU (no CPU timing exists)")
    dev = torch.device("cuda", 0)
    if "a" in a.part:
        part_a(a, dev)
        torch.cuda.empty_cache()
    if "b" in a.part:
        part_b(a, dev)


if __name__ == "__main__":
    main()
