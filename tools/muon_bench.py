"""Muon measurements on one GPU (figures: profiles/muon/README.md).

``ops.newton_schulz``'s launches on the 48 block matrices of GPT-2 small (2 prologue + 15 GEMM + 1 apply), captured
into a hipGraph once and replayed ``--rounds`` times ``--replays`` times between device events; the median is reported
with the flop rate of the iteration's 1.52 TFLOP.  ``--step`` adds the whole MuonMaster step over the same matrices,
alternating with the first arm.  (An arm that composed the recurrence from one ``torch.matmul`` per product under graph
capture is not part of this tool: see profiles/muon/README.md.)

    python tools/muon_bench.py [--layers 12] [--rounds 7] [--replays 5] [--step]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from pytorch_distributed_example_amd import ops  # noqa: E402
from pytorch_distributed_example_amd.optim import MuonMaster  # noqa: E402

SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]


def ns_flops(shapes, steps=5):
    return sum(steps * (2 * n * n * m + 2 * n * n * n + 2 * n * n * m)
               for n, m in ((min(s), max(s)) for s in shapes))


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def alternate(graphs, rounds, replays):
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, (g, _) in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / replays)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("muon_bench: needs a GPU")
    shapes = SHAPES * a.layers
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(*s, generator=g).bfloat16().cuda() for s in shapes]
    arms = {"newton_schulz": graph_of(lambda: ops.newton_schulz(xs))}
    if a.step:
        ps = [torch.nn.Parameter(x.clone() * 0.02) for x in xs]
        opt = MuonMaster(ps, capturable=True)
        opt.state_tensors()
        for p in ps:
            p.grad.normal_()
        arms["muon_step"] = graph_of(opt.step)
    res = alternate(arms, a.rounds, a.replays)
    # after the replays: the captured outputs hold the result (about 0.9 for a Gaussian input)
    norms = [round((o.float().norm() / min(o.shape) ** 0.5).item(), 4) for o in arms["newton_schulz"][1][:4]]
    fl = ns_flops(shapes)
    res["newton_schulz"]["tflops"] = fl / res["newton_schulz"]["median_ms"] * 1e-9
    out = {"matrices": len(shapes), "ns_flop": fl, "rms_singular_value_first4": norms, "times": res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
