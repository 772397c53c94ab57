"""FP8 forward (csrc/kernels/gemm_fp8.hip) on one MI355X: graph-replayed medians, A and B alternating in one call.

    python tools/fp8_gemm_bench.py [--tokens 16384] [--reps 7] [--iters 20] [--only gemm,quant,step] [--mx] [--out FILE]

* gemm:  the FP8 GEMM against ``gemm.fprop`` at the four GPT-2 block projections, alone and with the quantisation
         of the activation counted (the weights' share of one ``quantize_many`` per forward is reported apart);
* quant: the quantiser alone, one activation and the batched 48 block weights;
* step:  the captured GPT-2 training step (B = 16, T = 1024) with ``fp8_forward`` on against off.

``--mx`` adds the MXFP8 path (csrc/kernels/gemm_mxfp8.hip) to the same rounds: the block-scaled GEMM, ``k_mx_quant``,
the added time of the MX LayerNorm and of the ``act_mx`` epilogue over their plain forms, and the ``"mx"`` step.

Every figure is the median over ``--reps`` rounds of a graph holding ``--iters`` calls, timed with device events
after a warm-up replay; ``spread`` is (max - min) / median over the rounds.  FLOP/s use 2 M N K from the shapes.
One JSON line per measurement; there is no fallback without a GPU.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2  # noqa: E402
from pytorch_distributed_example_amd.ops import fp8  # noqa: E402
from pytorch_distributed_example_amd.ops import gemm as G  # noqa: E402
from pytorch_distributed_example_amd.ops import transformer as T  # noqa: E402
from pytorch_distributed_example_amd.optim import AdamWMaster  # noqa: E402

dev = "cuda"
SHAPES = {"c_attn": (2304, 768), "attn_proj": (768, 768), "c_fc+gelu": (3072, 768), "mlp_proj": (768, 3072)}


def capture(fn, iters):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def alternate(graphs, iters, reps):
    """{name: (median us per call, spread)} with the graphs replayed in turn inside every round."""
    us = {k: [] for k in graphs}
    for _ in range(reps):
        for k, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            us[k].append(s.elapsed_time(e) * 1e3 / iters)
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in us.items()}


def bench_gemm(M, iters, reps, emit, mx=False):
    for name, (N, K) in SHAPES.items():
        gelu = "gelu" in name
        x = torch.randn(M, K, device=dev).bfloat16()
        w = (0.02 * torch.randn(N, K, device=dev)).bfloat16()
        b = torch.zeros(N, device=dev, dtype=torch.bfloat16)
        xq, wq = fp8.quantize(x), fp8.quantize(w)
        cases = {"bf16": capture(lambda: G.fprop(x, w, b, gelu=gelu), iters),
                 "fp8": capture(lambda: fp8.fprop(xq, wq, b, gelu=gelu), iters),
                 "fp8+quant_x": capture(lambda: fp8.fprop(fp8.quantize(x), wq, b, gelu=gelu), iters)}
        if mx:
            xm, wm = fp8.quantize_mx(x), fp8.quantize_mx(w)
            cases["mxfp8"] = capture(lambda: fp8.fprop_mx(xm, wm, b, gelu=gelu), iters)
            if gelu:
                cases["mxfp8+act_mx"] = capture(lambda: fp8.fprop_mx(xm, wm, b, gelu=True, act_mx=True), iters)
        res = alternate(cases, iters, reps)
        row = {"what": "gemm", "proj": name, "M": M, "N": N, "K": K}
        for k, (us, spread) in res.items():
            row[k] = {"us": round(us, 2), "spread": round(spread, 3), "tflops": round(2.0 * M * N * K / us * 1e-6, 1)}
        emit(row)


def bench_quant(M, iters, reps, emit, mx=False):
    x = torch.randn(M, 768, device=dev).bfloat16()
    x4 = torch.randn(M, 3072, device=dev).bfloat16()
    ws = [(0.02 * torch.randn(N, K, device=dev)).bfloat16() for _ in range(12) for N, K in SHAPES.values()]
    cases = {"x[M,768]": capture(lambda: fp8.quantize(x), iters),
             "x[M,3072]": capture(lambda: fp8.quantize(x4), iters),
             "48 block weights, one call": capture(lambda: fp8.quantize_many(ws), iters),
             "48 block weights, 48 calls": capture(lambda: [fp8.quantize(w) for w in ws], iters)}
    nbytes = {"x[M,768]": 5 * x.numel(), "x[M,3072]": 5 * x4.numel()}      # read bf16 twice, write one byte
    if mx:                                                                  # MX: read bf16 once, write 1 + 1/32 bytes
        g, bt = torch.ones(768, device=dev).bfloat16(), torch.zeros(768, device=dev).bfloat16()
        cases.update({"mx x[M,768]": capture(lambda: fp8.quantize_mx(x), iters),
                      "mx x[M,3072]": capture(lambda: fp8.quantize_mx(x4), iters),
                      "mx 48 block weights, one call": capture(lambda: fp8.quantize_mx_many(ws), iters),
                      "add+ln [M,768]": capture(lambda: T.add_layer_norm_residual(x, x, g, bt), iters),
                      "add+ln [M,768] mx_out": capture(lambda: T.add_layer_norm_residual(x, x, g, bt, mx_out=True), iters)})
        mxb = lambda n: n * (3 + 1 / 32)
        nbytes.update({"mx x[M,768]": mxb(x.numel()), "mx x[M,3072]": mxb(x4.numel()),
                       "mx 48 block weights, one call": mxb(sum(w.numel() for w in ws)),
                       "add+ln [M,768]": 8 * x.numel(), "add+ln [M,768] mx_out": mxb(x.numel()) + 6 * x.numel()})
    res = alternate(cases, iters, reps)
    for k, (us, spread) in res.items():
        n = nbytes.get(k, 5 * sum(w.numel() for w in ws))
        emit({"what": "quant", "case": k, "us": round(us, 2), "spread": round(spread, 3),
              "GB/s": round(n / us * 1e-3, 1)})


def bench_step(reps, emit, mx=False, B=16, T=1024):
    graphs, keep = {}, []
    idx = torch.randint(0, 50257, (B, T), device=dev)
    tgt = torch.randint(0, 50257, (B, T), device=dev)
    ones = torch.ones((), device=dev)
    for name, kw in (("off", {}), ("on", {"fp8_forward": True}), ("mx", {"fp8_forward": True, "fp8_scaling": "mx"})):
        if name == "mx" and not mx:
            continue
        model = build_gpt2(GPTConfig(**kw), seed=0, device=dev)
        opt = AdamWMaster(model.decay_groups(0.1), lr=6e-4, betas=(0.9, 0.95), max_grad_norm=1.0, capturable=True)

        def step(model=model, opt=opt):
            opt.zero_grad()
            loss = model(idx, tgt)
            loss.backward(ones)
            opt.step()
            return loss.detach()

        graphs[name] = capture(step, 1)
        keep.append((model, opt))
    for _ in range(3):
        for g in graphs.values():
            g.replay()
    res = alternate(graphs, 1, reps)
    emit({"what": "step", "B": B, "T": T,
          **{f"fp8_forward {k}": {"ms": round(us * 1e-3, 3), "spread": round(sp, 3),
                                  "tokens/s": round(B * T / us * 1e6)} for k, (us, sp) in res.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="gemm,quant,step")
    ap.add_argument("--mx", action="store_true", help="add the MXFP8 path to the same rounds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_gemm_bench: needs a GPU (no figure is produced without one)")
    out = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    torch.manual_seed(0)
    only = a.only.split(",")
    if "gemm" in only:
        bench_gemm(a.tokens, a.iters, a.reps, emit, a.mx)
    if "quant" in only:
        bench_quant(a.tokens, a.iters, a.reps, emit, a.mx)
    if "step" in only:
        bench_step(a.reps, emit, a.mx)


if __name__ == "__main__":
    main()
