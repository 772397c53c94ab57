#!/usr/bin/env python3
"""GPT-2 small generation speed: ms per token of the KV-cache decode step in graph replay, against the
only way to generate without it -- ``model(window)[:, -1]``, a full forward over the context per token.

Per batch size (1 and 16) and 512 tokens of context, in one process:

* decode: a ``DecodeSession`` is prefilled with a 512-token prompt, its step is captured once, and windows
  of ``--window`` replays are timed (device events around the window and around every replay; the state is
  put back to position 512 before each window, so the context stays 512 .. 512 + window - 1).  The same
  step is also timed eagerly (host-launched) for comparison.
* recompute: ``model(idx[B, 512])[:, -1]`` eagerly under ``no_grad``, one event pair per call.

Achieved bytes/s of the decode step = (every parameter once in bf16, ``wte`` only through the LM head,
plus the K and V rows read, mean over the window) / median ms per token; compared with the 6.29 TB/s
achievable HBM bandwidth of MI355X_MICROARCH.md.  One JSON line per batch size.

Sampling is temperature 1.0 with ``--top-k`` (default 50, 0: none) and ``--top-p`` (default: off).  With
``--ragged`` the prompts of a batch have lengths spread evenly from 1 to ``--context`` (a batch of one keeps
``--context``), so the rows sit at different positions; the K / V bytes are then those of the rows' own
contexts.  ``--sampler-reps N`` also times the sampler launch alone (``k_sample`` and its one-thread tail) on
the logits of the prefill: N back-to-back calls between one event pair, with the run's settings and with
top-p off.  ``--penalties`` adds a second row per batch size, from the same process and prompt: the same step
with the logit processors on (``repetition_penalty`` 1.3, ``frequency_penalty`` 0.3, ``presence_penalty`` 0.5 and
a ``[V]`` logit bias), and under ``--sampler-reps`` the sampler launch with them (the ``PROC`` instantiation).
``--history`` adds a row with the history constraints on (``no_repeat_ngram_size`` 3 and two stop sequences that
never match, so every row stays live and is scanned at every step; on top of the penalties under ``--penalties``),
and under ``--sampler-reps`` the sampler launch with them (the ``HIST`` instantiation) on a 512-token history.
``--beams K`` adds a row with beam search: ``--batch-sizes`` then counts physical rows ``R`` (a multiple of ``K``), the
plain row runs ``R`` sampled sequences and the beam row ``R / K`` prompts with ``K`` beams each -- the same number of
rows through the same step, with the table-indirect attention and the beam selection in place of the plain attention
and the sampler -- and under ``--sampler-reps`` the beam step's three launches alone, on ``randn * 3`` logits and on rows whose logits
are all equal (every candidate a tie at the threshold: the selection's worst case).

    python tools/gpt2_decode_bench.py [--context 512] [--window 64] [--rounds 5] [--batch-sizes 1 16]
                                      [--top-k 50] [--top-p P] [--ragged] [--sampler-reps N] [--penalties]
                                      [--history] [--beams K]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2  # noqa: E402
from pytorch_distributed_example_amd.models.gpt2 import DecodeSession  # noqa: E402
from pytorch_distributed_example_amd.ops import DeviceRNG  # noqa: E402
from pytorch_distributed_example_amd.ops import decode as D  # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def events(n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def prompt_lens(B, context):
    """Lengths spread evenly from 1 to ``context``"""
    return [context] if B == 1 else [1 + round(b * (context - 1) / (B - 1)) for b in range(B)]


def penalty_processors(cfg, dev):
    """The processors of the ``--penalties`` row"""
    bias = 0.5 * torch.randn(cfg.vocab_size, device=dev, generator=torch.Generator(dev).manual_seed(7))
    return D.LogitProcessors(repetition_penalty=1.3, frequency_penalty=0.3, presence_penalty=0.5, logit_bias=bias)


def history_constraints(cfg):
    """The constraints of the ``--history`` row; 50256 ends no stop sequence of the random prompt's tokens"""
    return D.HistoryConstraints(no_repeat_ngram_size=3, stop_sequences=[[198, 198, 50256], [628, 50256]],
                                eos_token_id=cfg.vocab_size - 2)


def bench_sampler(B, cfg, top_k, top_p, reps, dev, procs=None, hist=None, context=512):
    """us per sampler launch (k_sample + tail), ``reps`` calls between one event pair"""
    logits = (torch.randn(B, cfg.padded_vocab, device=dev) * 3).to(torch.bfloat16)
    state = D.DecodeState(dev, DeviceRNG(0, device=dev).state)
    nxt = torch.zeros(B, device=dev, dtype=torch.int64)
    out = torch.zeros(B, 1, device=dev, dtype=torch.int64)
    kw = {}
    if hist is not None:             # a history of `context` tokens; the step advances, so leave room for the calls
        out = torch.randint(0, cfg.vocab_size - 2, (B, context + reps + 11), device=dev)
        procs = D.LogitProcessors(eos_token_id=hist.eos_token_id) if procs is None else procs
        kw = dict(history=hist, stop_hit=torch.full((B,), -1, device=dev, dtype=torch.int32), T0=context)
    if procs is not None:            # buffers allocated once, as a generation does
        kw = dict(kw, processors=procs, counts=D.TokenCounts(B, cfg.padded_vocab, dev),
                  processed_out=torch.empty_like(logits), _bias=procs.bias(B, cfg.vocab_size, cfg.padded_vocab, dev))
    for _ in range(10):
        D.sample(logits, cfg.vocab_size, state, 1.0, top_k, next=nxt, out=out, top_p=top_p, **kw)
    e0, e1 = events(1)[0]
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        D.sample(logits, cfg.vocab_size, state, 1.0, top_k, next=nxt, out=out, top_p=top_p, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def bench_beam_step(B, K, cfg, reps, dev, context=512, all_equal=False):
    """us per beam step (k_beam_rows, k_beam_merge and the tail), ``reps`` calls between one event pair; the table
    copy is that of a row at position ``context`` and beyond.  ``all_equal``: every logit the same value, the
    selection's worst case -- all ``K`` of a row's candidates are ties at the threshold, one pass over the row each"""
    logits = (torch.randn(B * K, cfg.padded_vocab, device=dev) * 3).to(torch.bfloat16)
    if all_equal:
        logits.fill_(0.75)
    bb = D.BeamBuffers(D.BeamConfig(K), torch.zeros(B, context, device=dev, dtype=torch.int64), None, 1,
                       cfg.vocab_size, cfg.padded_vocab, dev, context + reps + 11)
    bb.state.reset(pos=context, step=1)
    for _ in range(10):
        bb.sample(logits)
    e0, e1 = events(1)[0]
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        bb.sample(logits)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def bench_decode(model, idx, a, lens=None, procs=None, hist=None, beams=0):
    if beams:
        ses = DecodeSession(model, idx, a.window + 1, prompt_lens=lens, beam=D.BeamConfig(beams))
    else:
        ses = DecodeSession(model, idx, a.window + 1, 1.0, a.top_k or None, DeviceRNG(0, device=idx.device).state,
                            eos=None if hist is None else hist.eos_token_id, top_p=a.top_p, prompt_lens=lens,
                            processors=procs, history=hist)
    graph = ses.capture()
    start = (ses.state.buf.clone(), ses.next.clone(), None if ses.counts is None else ses.counts.buf.clone())
    beam_start = ses.buffers.snapshot() if beams else None

    def rewind():
        if beams:        # S, len and the state; the table keeps whatever rows of the group the last window left
            ses.buffers.restore(beam_start)
            return
        ses.state.buf.copy_(start[0])
        ses.next.copy_(start[1])
        if start[2] is not None:
            ses.counts.buf.copy_(start[2])
        if ses.stop_hit is not None:
            ses.stop_hit.fill_(-1)

    per_replay, per_window, eager = [], [], []
    for r in range(a.rounds + 1):                       # round 0 is warm-up
        rewind()
        ev, (w0, w1) = events(a.window), events(1)[0]
        torch.cuda.synchronize()
        w0.record()
        for s, e in ev:
            s.record()
            graph.replay()
            e.record()
        w1.record()
        torch.cuda.synchronize()
        if r:
            per_replay += [s.elapsed_time(e) for s, e in ev]
            per_window.append(w0.elapsed_time(w1) / a.window)
        rewind()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.window):
            ses.step()
        torch.cuda.synchronize()
        if r:
            eager.append((time.perf_counter() - t0) * 1e3 / a.window)
    return per_replay, per_window, eager


def bench_recompute(model, idx, reps):
    for _ in range(3):
        model(idx)[:, -1]
    ev = events(reps)
    torch.cuda.synchronize()
    for s, e in ev:
        s.record()
        model(idx)[:, -1]
        e.record()
    torch.cuda.synchronize()
    return [s.elapsed_time(e) for s, e in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--recompute-reps", type=int, default=20, help="0: skip the recompute baseline")
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--top-k", type=int, default=50, help="0: no top-k")
    ap.add_argument("--top-p", type=float, default=None, help="nucleus mass in (0, 1]; default: off")
    ap.add_argument("--ragged", action="store_true", help="prompt lengths spread from 1 to --context")
    ap.add_argument("--sampler-reps", type=int, default=0, help="also time the sampler launch alone")
    ap.add_argument("--penalties", action="store_true", help="a second row per batch size with the logit processors on")
    ap.add_argument("--history", action="store_true", help="a further row with the history constraints on")
    ap.add_argument("--beams", type=int, default=0, help="a further row with beam search: batch size / K prompts x K beams")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpt2_decode_bench: needs a GPU (no CPU fallback: a CPU time says nothing about the kernels)")
    dev = torch.device("cuda", 0)
    cfg = GPTConfig()
    model = build_gpt2(cfg, seed=0, device=dev).eval()
    weight_bytes = 2 * sum(p.numel() for p in model.parameters())
    with torch.no_grad():
        for B in a.batch_sizes:
            idx = torch.randint(0, cfg.vocab_size, (B, a.context), device=dev,
                                generator=torch.Generator(dev).manual_seed(B))
            lens = prompt_lens(B, a.context) if a.ragged else None
            rec = None
            # keys read at positions len .. len + window - 1, summed over the rows
            mean_keys = sum(n + (a.window + 1) / 2.0 for n in (lens or [a.context] * B))
            kv_bytes = cfg.n_layer * 2 * cfg.n_head * mean_keys * 64 * 2
            pen = penalty_processors(cfg, dev) if a.penalties else None
            rows = [(None, None, 0)] + ([(pen, None, 0)] if a.penalties else [])
            rows += [(pen, history_constraints(cfg), 0)] if a.history else []
            if a.beams:
                if a.beams < 2 or B % a.beams:
                    sys.exit(f"gpt2_decode_bench: --beams {a.beams} needs batch sizes that are multiples of it (got {B})")
                rows.append((None, None, a.beams))
            for procs, hist, beams in rows:
                nb = B // beams if beams else B              # prompts of this row
                per_replay, per_window, eager = bench_decode(model, idx[:nb], a, lens and lens[::beams or 1], procs,
                                                             hist, beams)
                if procs is None and hist is None and a.recompute_reps > 0:   # once per batch size, after the plain row
                    rec = bench_recompute(model, idx, a.recompute_reps)
                extra = {"top_k": a.top_k, "top_p": a.top_p, "prompt_lens": lens, "penalties": procs is not None,
                         "history": hist is not None, "num_beams": beams or 1, "prompts": nb}
                if a.sampler_reps > 0 and beams:
                    extra["beam_step_us_per_launch"] = {
                        "randn_x3": round(bench_beam_step(nb, beams, cfg, a.sampler_reps, dev, a.context), 2),
                        "all_equal": round(bench_beam_step(nb, beams, cfg, a.sampler_reps, dev, a.context, True), 2)}
                elif a.sampler_reps > 0:
                    k = a.top_k or None
                    args = (a.sampler_reps, dev, procs, hist, a.context)
                    extra["sampler_us_per_launch"] = {
                        "this_run": round(bench_sampler(B, cfg, k, a.top_p, *args), 2),
                        "top_p_off": round(bench_sampler(B, cfg, k, None, *args), 2)}
                ms = statistics.median(per_replay)
                bps = (weight_bytes + kv_bytes) / (ms * 1e-3)
                print(json.dumps({
                    "metric": "gpt2_small_decode_ms_per_token", "batch_size": B, "context": a.context,
                    "window": a.window, "rounds": a.rounds,
                    "decode_graph_ms_per_token": {"median": round(ms, 4), "min": round(min(per_replay), 4),
                                                  "max": round(max(per_replay), 4),
                                                  "window_mean_median": round(statistics.median(per_window), 4)},
                    "decode_eager_ms_per_token_median": round(statistics.median(eager), 4),
                    "recompute_forward_ms_per_token": rec and {"median": round(statistics.median(rec), 4),
                                                               "min": round(min(rec), 4), "max": round(max(rec), 4)},
                    "speedup_vs_recompute": rec and round(statistics.median(rec) / ms, 2),
                    "tokens_per_s_decode": round(B / (ms * 1e-3), 1),
                    "bytes_per_token": {"weights": weight_bytes, "kv": int(kv_bytes)},
                    "achieved_bytes_per_s": round(bps, 1),
                    "share_of_6.29TBps": round(bps / HBM_BYTES_PER_S, 4), **extra}), flush=True)

if __name__ == "__main__":
    main()
