"""Inputs shared by ``test_speculative_cpu.py`` and ``test_speculative_gpu.py``: hand-made verify steps whose outcome
is written down here (the CPU test holds the twins to it, the GPU test the kernels to the twins), and the tiny models of
the end-to-end tests."""
import torch

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2

V, VP, EOS, K, NGRAM, MAX_NEW = 9001, 9216, 7, 3, 3, 12      # Vp / 8 > 1024: more than one load per thread
_P = [10, 11, 12, 13, 14, 15]


def _long_prompt():
    """1500 tokens (longer than a block) without 1, 2, 3 except where planted: ``1 2 3`` at 200 and again at 900."""
    h = torch.randint(100, 9000, (1500,), generator=torch.Generator().manual_seed(3)).tolist()
    h[200:204] = [1, 2, 3, 4]
    h[900:906] = [1, 2, 3, 5, 6, 8]
    return h


# name -> prompt, tokens generated so far, g_0 .. g_K, the drafts d_1 .. d_K in flight; then what the step must do:
# the tokens it emits, whether the group is finished, and (if not) the drafts for the next step
HAND = {
    "accept_all": (_P, [20], [21, 22, 23, 24], [21, 22, 23], [21, 22, 23, 24], False, [24, 24, 24]),
    "accept_none_no_match": (_P, [20], [21, 22, 23, 24], [30, 22, 23], [21], False, [21, 21, 21]),
    "partial_prefix": (_P, [20], [21, 22, 23, 24], [21, 31, 23], [21, 22], False, [22, 22, 22]),
    "eos_inside": (_P, [20], [21, EOS, 23, 24], [21, EOS, 23], [21, EOS], True, None),
    "budget_cut": (_P, list(range(40, 50)), [21, 22, 23, 24], [21, 22, 23], [21, 22], True, None),
    "match_3": (_P, [20], [11, 12, 13, 99], [11, 12, 50], [11, 12, 13], False, [14, 15, 20]),
    "match_1_only": (_P, [20], [21, 13, 98, 99], [21, 60, 98], [21, 13], False, [14, 15, 20]),
    # two tokens of budget left afterwards: draft rows 2 and 3 are idle, parked on row 0
    "idle_rows": (_P, list(range(40, 49)), [12, 22, 23, 24], [30, 22, 23], [12], False, [13, 14, 15]),
    "period_2":([5, 6, 5], [6], [5, 70, 71, 72], [80, 70, 71], [5], False, [6, 5, 6]),
    "long_history": (_long_prompt(), [1, 2], [3, 97, 98, 99], [0, 97, 98], [3], False, [5, 6, 8]),
}
BATCHES = [list(HAND)[i:i + 4] for i in range(0, len(HAND), 4)]      # 4 groups x 4 rows: all 16 rows of a step


def tiny_cfg():
    return GPTConfig(block_size=256, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128)


def repeating_model(device, dtype, seed=5):
    """``wpe`` and every block's two ``c_proj`` (weights and biases) zeroed: the residual stream is the token embedding
    whatever the position, so every step sees the logits of its own token alone."""
    g = build_gpt2(tiny_cfg(), seed=seed, device=device, dtype=dtype)
    with torch.no_grad():
        g.transformer.wpe.weight.zero_()
        for blk in g.transformer.h:
            for lin in (blk.attn.c_proj, blk.mlp.c_proj):
                lin.weight.zero_()
                lin.bias.zero_()
    return g


REPEAT_PROMPT = torch.tensor([[3, 141, 59, 26, 535]])
REPEAT_NEW = 33
