"""Inputs shared by ``test_beam_search_cpu.py`` and ``test_beam_search_gpu.py``, so that the input conditions checked
on the CPU are those of the very tensors the GPU tests feed to the kernels."""
import functools

import torch

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.ops import decode as D

import generate_cases as GC

BF16 = torch.bfloat16
GAP = GC.GAP              # 1e-4: below it the device selection may differ from the fp64 reference's
MIN_GAP = 1e-3            # what the CPU file asserts of every input below: the GPU comparison is exact
EOS = 7

# ------------------------------------------------------------------------------------------- kernel inputs
KERNEL_SHAPES = [(1, 1, 1000, 1024), (2, 8, 50257, 50304), (1, 16, 50257, 50304), (4, 4, 1000, 1024),
                 (3, 5, 1000, 1024), (5, 3, 50257, 50304)]       # (B, K, V, Vp)
N_KERNEL_INPUTS = 6


def kernel_input(i, B, K, V, Vp):
    """``(logits [B*K, Vp] bf16, S [B*K] fp32, finished [B*K] bool)``; rows with ``r % 5 == 1`` are finished."""
    g = torch.Generator().manual_seed(4000 + 10 * i + B * K + V)
    logits = (torch.randn(B * K, Vp, generator=g) * 3).to(BF16)
    S = -(torch.rand(B * K, generator=g) * 4)
    fin = torch.arange(B * K) % 5 == 1
    return logits, S, fin


@functools.lru_cache(maxsize=None)
def kernel_reference(i, B, K, V, Vp):
    """``(parent, tok, score, info)`` of ``beam_step_reference`` on ``kernel_input``, computed once."""
    logits, S, fin = kernel_input(i, B, K, V, Vp)
    return D.beam_step_reference(logits, V, K, S, fin, EOS, return_info=True)


# ------------------------------------------------------------------------------------------- hand-made steps
def hand_cases():
    """name -> dict(B, K, V, Vp, logits, S, fin, len, first): one beam step each, eos = ``EOS``."""
    V, Vp = 1000, 1024
    g = torch.Generator().manual_seed(99)
    rnd = lambda R: (torch.randn(R, Vp, generator=g) * 3).to(BF16)      # noqa: E731
    cases = {}
    # every logit of every row equal: beam 0 (the best S) supplies all K, tokens 0 .. K-1 by index
    cases["all_equal"] = dict(B=1, K=4, logits=torch.full((4, Vp), 0.75).to(BF16), S=[-0.5, -1.0, -2.0, -3.0],
                              fin=[0, 0, 0, 0], len=[3, 3, 3, 3])
    # step 0: only row b * K exists; the other rows hold values that would win if they were read
    lg = rnd(6)
    lg[1:3] = 60.0
    lg[4:6] = 60.0
    cases["step0"] = dict(B=2, K=3, logits=lg, S=[0.0] * 6, fin=[0] * 6, len=[0] * 6, first=True)
    # a group whose beams are all finished: order by S, scores and lengths preserved, every token eos
    cases["all_finished"] = dict(B=1, K=4, logits=rnd(4), S=[-3.0, -1.0, -2.0, -4.0], fin=[1, 1, 1, 1],
                                 len=[2, 5, 3, 4])
    # two beams with the same S and the same row: an exact cross-beam tie, the lower beam first
    row = rnd(1)
    cases["cross_beam_tie"] = dict(B=1, K=2, logits=row.repeat(2, 1), S=[-1.25, -1.25], fin=[0, 0], len=[2, 2])
    # a live beam whose best token is eos becomes finished and its len counts the eos; a frozen beam's does not grow
    lg = rnd(3)
    lg[0, EOS] = 40.0
    cases["chooses_eos"] = dict(B=1, K=3, logits=lg, S=[-0.5, -0.75, -9.0], fin=[0, 1, 0], len=[4, 2, 4])
    for c in cases.values():
        c.update(V=V, Vp=Vp)
        c.setdefault("first", False)
    return cases


def hand_reference(c):
    return D.beam_step_reference(c["logits"], c["V"], c["K"], torch.tensor(c["S"]), torch.tensor(c["fin"]).bool(), EOS,
                                 first=c["first"], return_info=True)


# ------------------------------------------------------------------------------------------- whole model
LN_F_SCALE = 13.25        # bf16-representable; the untrained model's logits then spread like randn * 3


@functools.lru_cache(maxsize=None)
def twin():
    """The fp32 CPU twin of the GPU tests' bf16 model: ``tiny_cfg``, seed 0, bf16-representable weights, ``ln_f.weight``
    scaled so that a row's logits do not tie massively in bf16."""
    m = build_gpt2(GC.tiny_cfg(), seed=0, dtype=BF16)
    with torch.no_grad():
        m.transformer.ln_f.weight.fill_(LN_F_SCALE)
    return m.float().eval()


# (B, K, T0, n_new, prompt seed); the seeds are chosen so that the twin's own generation has no step whose gap is
# below MIN_GAP (asserted in the CPU file)
HYP_CASES = [(2, 4, 5, 6, 0), (2, 4, 130, 3, 0), (1, 3, 120, 140, 0)]
RAGGED_LENS, RAGGED_K, RAGGED_NEW, RAGGED_SEED = [7, 1, 130], 4, 5, 0


def prompt(B, T0, seed):
    return torch.randint(0, 1000, (B, T0), generator=torch.Generator().manual_seed(1000 * seed + 10 * T0 + B))


def step_gaps(model, idx, n_new, K, **kw):
    """The per-step, per-prompt gaps ``[n_new, B]`` of ``model``'s own CPU beam search from ``idx``."""
    tr = {}
    model.generate(idx, n_new, num_beams=K, _beam_trace=tr, **kw)
    return tr["gap"]
