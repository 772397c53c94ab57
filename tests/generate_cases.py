"""Inputs shared by ``test_generate_ragged_cpu.py`` and ``test_generate_ragged_gpu.py``, so that the input
conditions checked on the CPU are those of the very tensors the GPU tests feed to the kernels."""
import numpy as np
import torch

from pytorch_distributed_example_amd.models import GPTConfig
from pytorch_distributed_example_amd.ops import DeviceRNG

from test_generate_gpu import sampler_logits  # noqa: F401  (the existing sampler inputs)

SAMPLER_SHAPES = [(B, V, Vp) for (V, Vp) in ((1000, 1024), (50257, 50304)) for B in (1, 5, 16)]
TOPP_SETTINGS = [(t, k, p) for t in (0.7, 1.0) for k in (None, 50) for p in (0.9, 0.5, 0.05)]
N_TOPP_CASES = sum(B for B, _, _ in SAMPLER_SHAPES) * len(TOPP_SETTINGS)      # (row, setting) pairs: 528
P_SLACK = 1e-4            # below it the device threshold may sit anywhere in threshold_p_bracket
MAX_CLOSE_CASES = 16      # ... and at most this many of the 528 cases may be that close
GAP = 1e-4                # the existing sampler test's bound on best minus runner-up


def topp_seed(B, V, i):
    """Chosen so that no row's best-versus-runner-up gap is below ``GAP`` (checked on the CPU)."""
    return 5200 + 1000 * i + 10 * B + V


def topp_snapshot(B, V, i):
    return DeviceRNG(topp_seed(B, V, i)).next()


def tiny_cfg():
    return GPTConfig(block_size=512, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128)


def ragged_prompt(lens, width=None, seed=None):
    """``[B, width]`` tokens (``width`` defaults to ``max(lens)``).  The columns past a row's length hold
    random tokens too -- ``generate`` has to ignore them -- and ``unpadded(idx, lens)`` are the prompts."""
    width = max(lens) if width is None else width
    g = torch.Generator().manual_seed(sum(lens) if seed is None else seed)
    return torch.randint(0, 1000, (len(lens), width), generator=g)


# the hand-made nucleus row: probabilities whose logits are their logs, V = 16
HAND_P = np.array([0.4, 0.3, 0.1, 0.1, 0.05] + [0.05 / 11] * 11)


def hand_row(n):
    return torch.from_numpy(np.log(HAND_P)).float().repeat(n, 1)
