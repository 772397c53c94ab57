"""The logit processors' definition as plain loops over ``(b, v)``, and the inputs shared by
``test_logit_processors_cpu.py`` and ``test_logit_processors_gpu.py``, so that the conditions checked on the CPU
are those of the very tensors the GPU tests feed to the kernel.

``loops`` computes in Python floats (fp64) and rounds every operation to fp32 through ``numpy.float32``: a
product of two fp32 numbers is exact in fp64 and a sum or difference is rounded to 53 bits first, which for
``53 >= 2 * 24 + 2`` cannot change the fp32 rounding, so every line is the correctly rounded fp32 operation."""
import math

import numpy as np
import torch

from pytorch_distributed_example_amd.ops import DeviceRNG, LogitProcessors, TokenCounts

PROMPT, COUNT = 1 << 30, (1 << 30) - 1
SHAPES = [(1, 1000, 1024), (5, 997, 1000), (16, 50257, 50304)]
STEP = 2                                  # the generation step of the kernel tests: below MIN_NEW
MIN_NEW = 3
GAP = 1e-4                                # the existing sampler tests' bound on best minus runner-up
P_SLACK = 1e-4                            # ... and on the distance of top_p * W from a threshold boundary
SETTINGS = [(0.0, None, None), (0.8, 40, None), (1.0, None, 0.9), (0.7, 50, 0.5)]


def f32(x, _f=np.float32):
    return float(_f(x))


def loops(logits, V, counts, r=1.0, f=0.0, p=0.0, bias=None, m=0, eos=None, step=0):
    """``logits`` ``[B, Vp]`` (torch, any float dtype), ``counts`` int32 ``[B, Vp]``, ``bias`` ``None`` or fp32
    ``[1 or B, >= V]`` -> ``[B, Vp]`` in the logits' dtype, the columns ``>= V`` untouched."""
    xs = logits.float().tolist()
    cs = counts.tolist()
    bs = None if bias is None else bias.tolist()
    r32, inv_r, f_, p_ = f32(r), f32(1.0 / r), f32(f), f32(p)
    out = []
    for b in range(len(xs)):                 # no overflow: |x| <= 3e5 here
        xb, cb = xs[b], cs[b]
        bb = None if bs is None else bs[b if len(bs) > 1 else 0]
        row = []
        for v in range(V):
            x, c = xb[v], cb[v]
            n = c & COUNT
            if c != 0:
                x = f32(x * inv_r) if x > 0 else f32(x * r32)
            t = f32(f_ * f32(n))
            x = f32(x - t)
            x = f32(x - (p_ if n > 0 else 0.0))
            if bb is not None:
                x = f32(x + bb[v])
            if step < m and v == eos:
                x = -math.inf
            row.append(x)
        out.append(row)
    y = logits.clone()
    y[:, :V] = torch.tensor(out, dtype=torch.float64).to(torch.float32).to(logits.dtype)
    return y


def fused_variant(logits, V, counts, r=1.0, f=0.0, p=0.0):
    """Steps 1, 2 and 5 with step 2's ``x - f * n`` contracted: the product kept exact (fp64), one rounding."""
    x = logits.float().numpy()[:, :V].astype(np.float32)
    c = counts.numpy()[:, :V]
    n = c & COUNT
    x = np.where(c != 0, np.where(x > 0, x * np.float32(1.0 / r), x * np.float32(r)), x)
    prod = np.float64(np.float32(f)) * n.astype(np.float32).astype(np.float64)
    x = (x.astype(np.float64) - prod).astype(np.float32)
    x = x - np.where(n > 0, np.float32(p), np.float32(0))
    y = logits.clone()
    y[:, :V] = torch.from_numpy(x).to(logits.dtype)
    return y


# --------------------------------------------------------------------------------------- inputs
# added to the logits' seed per shape: chosen on the CPU so that under the top-p settings every row's target mass is
# at least P_SLACK away from a threshold boundary (test_logit_processors_cpu.py checks it)
LOGITS_BUMP = {(1, 1000): 1, (5, 997): 3, (16, 50257): 6}


def make_logits(B, V, Vp, dtype=torch.bfloat16):
    """randn * 3 (positives and negatives) with +0 and -0 planted in every row."""
    g = torch.Generator().manual_seed(4000 + B + V + LOGITS_BUMP.get((B, V), 0))
    lg = (torch.randn(B, Vp, generator=g) * 3).to(dtype)
    lg[:, 3] = 0.0
    lg[:, 4] = -0.0
    lg[:, V - 1] = -0.0
    return lg


def make_counts(B, V, Vp):
    """About half of the entries ``< V`` hold a count in 1..5, a quarter of all entries carry the prompt flag
    (with and without a count), one entry holds 70000; the pad columns are zero."""
    g = torch.Generator().manual_seed(4100 + B + V)
    n = torch.randint(1, 6, (B, Vp), generator=g, dtype=torch.int32)
    n = torch.where(torch.rand(B, Vp, generator=g) < 0.5, n, torch.zeros_like(n))
    flag = (torch.rand(B, Vp, generator=g) < 0.25).int() * PROMPT
    c = n | flag
    c[0, 3], c[0, 4] = 2, 1                 # the zeros of row 0: penalised from +0 and from -0
    c[B - 1, 7] = 70000
    c[:, V:] = 0
    return c.to(torch.int32)


def make_bias(B, V, per_row):
    g = torch.Generator().manual_seed(4200 + B + V + int(per_row))
    bias = torch.randn(B if per_row else 1, V, generator=g)
    bias[:, 11] = -math.inf
    bias[0, V - 2] = -math.inf
    return bias if per_row else bias[0]          # [B, V] or [V]


def eos_of(V):
    return V - 5


SUPPRESS = [0, 17, 500]

# each processor alone and all together: keyword sets for ``LogitProcessors`` / ``loops``
CASES = {
    "repetition": dict(r=1.3),
    "repetition<1": dict(r=0.7),
    "frequency": dict(f=0.3),
    "presence": dict(p=0.5),
    "bias": dict(bias="shared"),
    "bias_rows": dict(bias="rows"),
    "suppress": dict(suppress=True),
    "min_new": dict(m=MIN_NEW),
    "frequency+presence": dict(f=0.3, p=0.5),     # the case in which a fused multiply-add shows (see the CPU test)
    "all": dict(r=1.3, f=0.3, p=0.5, bias="rows", suppress=True, m=MIN_NEW),
}


def make_case(name, B, V, device="cpu"):
    """``(LogitProcessors, keywords of loops)`` of a case; the processors' bias lives on ``device``."""
    c = CASES[name]
    bias = make_bias(B, V, c["bias"] == "rows") if c.get("bias") else None
    m = c.get("m", 0)
    eos = eos_of(V) if m else None
    procs = LogitProcessors(c.get("r", 1.0), c.get("f", 0.0), c.get("p", 0.0),
                            None if bias is None else bias.to(device), SUPPRESS if c.get("suppress") else None, m, eos)
    merged = None if bias is None else bias.reshape(-1, V)
    if c.get("suppress"):
        merged = torch.zeros(1, V) if bias is None else merged.clone()
        merged[:, SUPPRESS] = -math.inf
    return procs, dict(r=c.get("r", 1.0), f=c.get("f", 0.0), p=c.get("p", 0.0), bias=merged, m=m, eos=eos)


def token_counts(B, V, Vp, device="cpu"):
    tc = TokenCounts(B, Vp, device)
    tc.buf.copy_(make_counts(B, V, Vp))
    return tc


# seeds of the kernel-against-twin test, per (shape, setting): with them the reference's own gap is >= GAP on every
# row (test_logit_processors_cpu.py checks it)
def twin_seed(B, V, i):
    return 9100 + 1000 * i + 10 * B + V


def twin_snapshot(B, V, i):
    return DeviceRNG(twin_seed(B, V, i)).next()


# --------------------------------------------------------------------------------------- a generation, replayed
def replay_generation(out, raw, idx, lens, V, Vp, procs, seed, temperature, top_k, top_p, eos):
    """Check a finished generation from its own outputs.  ``out`` are the returned tokens, ``raw`` the returned
    raw logits ``[B, n_new, V]``, ``idx`` / ``lens`` the prompts (``lens`` ``None``: one length).  For every step
    the counts are rebuilt on the host from the prompt and the tokens returned so far, the raw logits are processed
    with the twin and sampled with the step's snapshot.  Returns ``(mismatches, close)``: the ``(b, s)`` where the
    returned token differs from the twin's although the twin's gap is at least ``GAP``, and the number of rows and
    steps closer than that."""
    from pytorch_distributed_example_amd.ops import process_logits_reference, sample_reference
    out, raw, idx = out.cpu(), raw.cpu(), idx.cpu()
    B, n_new = raw.shape[:2]
    lens = [idx.shape[1]] * B if lens is None else list(lens)
    counts = torch.zeros(B, Vp, dtype=torch.int32)
    for b, n in enumerate(lens):
        for t in range(n):
            counts[b, int(idx[b, t])] = PROMPT
    rng = DeviceRNG(seed)
    fin = torch.zeros(B, dtype=torch.bool)
    rows = torch.arange(B)
    mismatches, close = [], 0
    for s in range(n_new):
        lg = torch.zeros(B, Vp, dtype=raw.dtype)
        lg[:, :V] = raw[:, s]
        y = process_logits_reference(lg, V, counts, procs, s)
        ref, info = sample_reference(y, V, rng.next(), temperature, top_k, top_p=top_p, return_info=True)
        got = out[rows, torch.tensor(lens) + s]
        if eos is not None:
            ref = torch.where(fin, torch.full_like(ref, eos), ref)
        near = torch.from_numpy(info["gap"] < GAP) & ~fin
        close += int(near.sum())
        mismatches += [(b, s, int(got[b]), int(ref[b])) for b in range(B) if got[b] != ref[b] and not near[b]]
        if eos is not None:
            fin = fin | (got == eos)
        counts[rows, got] += 1                    # the history is what the generation returned
    return mismatches, close
