"""Speculative decoding, the CPU side: the drafting and acceptance twins against steps worked out by hand and against
loops written out, the trace replay on sequences whose trace is known, and ``GPT.generate(num_draft_tokens=)`` on CPU
tensors, which is the plain greedy loop by definition."""
import random

import pytest
import torch

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.ops import decode as D

import spec_cases as SC


@pytest.mark.parametrize("name", list(SC.HAND))
def test_twins_on_hand_made_steps(name):
    prompt, gen, greedy, drafts, emit, fin, nxt = SC.HAND[name]
    assert D.spec_accept_reference(greedy, drafts, len(gen), SC.MAX_NEW, SC.EOS) == (emit, fin)
    if not fin:
        assert D.draft_reference(prompt + gen + emit, SC.K, SC.NGRAM) == nxt


def _draft_loops(h, K, ngram):
    """The rule with every (m, j) pair enumerated: the longest m first, then the latest j."""
    L = len(h)
    pairs = [(m, j) for m in range(1, min(ngram, L - 1) + 1) for j in range(m - 1, L - 1)
             if all(h[j - t] == h[L - 1 - t] for t in range(m))]
    if not pairs:
        return [h[-1]] * K
    j = max(pairs)[1]
    cont = h[j + 1:]                            # the history continues with this, over and over
    return [cont[(i - 1) % len(cont)] for i in range(1, K + 1)]


def test_twins_against_loops_written_out():
    rnd = random.Random(0)
    for _ in range(300):
        h = [rnd.randrange(3) for _ in range(rnd.randrange(1, 14))]
        K, ngram = rnd.randrange(1, 8), rnd.randrange(1, 5)
        assert D.draft_reference(h, K, ngram) == _draft_loops(h, K, ngram), (h, K, ngram)
        g, d = [rnd.randrange(3) for _ in range(K + 1)], [rnd.randrange(3) for _ in range(K)]
        budget = rnd.randrange(1, 6)
        n = rnd.randrange(budget)
        emit = []
        for i in range(K + 1):                  # g_i is emitted while every draft before it was right
            if i > 0 and d[i - 1] != g[i - 1]:
                break
            emit.append(g[i])
            if len(emit) == budget - n or g[i] == 2:
                break
        assert D.spec_accept_reference(g, d, n, budget, 2) == (emit, 2 in emit or n + len(emit) == budget)


def test_trace_of_known_sequences():
    # 1 2 3 | 1 2 3 1 2 3 1: the prefill gives the first 1; lookup finds it at j = 0 and proposes 2 3 1, all right; the
    # next step has two tokens of budget left
    a = [1, 2, 3, 1, 2, 3, 1, 2, 3, 1]
    steps, acc = D.spec_trace_reference([a], [3], 7, 3)
    assert steps == 2 and acc.tolist() == [[3], [1]]
    # no repetition: every step drafts its own last token and is wrong, n_new - 1 steps
    b = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    steps, acc = D.spec_trace_reference([b], [3], 7, 3)
    assert steps == 6 and acc.sum().item() == 0
    # together: the groups finish at different steps; and an eos (9) stops the second group early
    steps, acc = D.spec_trace_reference([a, b], [3, 3], 7, 3)
    assert steps == 6 and acc.sum(0).tolist() == [4, 0] and acc[2:, 0].sum().item() == 0
    c = b[:6] + [9] * 4
    steps, acc = D.spec_trace_reference([a, c], [3, 3], 7, 3, eos=9)
    assert steps == 3 and acc.sum(0).tolist() == [4, 0]      # 4 | 5 | 6 | 9: the prefill's token and three steps


def test_generate_on_the_cpu_is_the_plain_greedy_loop():
    g = build_gpt2(SC.tiny_cfg(), seed=1, device="cpu", dtype=torch.float32)
    idx = torch.randint(0, 1000, (2, 9), generator=torch.Generator().manual_seed(2))
    for kw in (dict(), dict(prompt_lens=[9, 5], eos_token_id=3)):
        plain, lp = g.generate(idx, 10, temperature=0.0, return_logits=True, **kw)
        stats = {}
        out, lg = g.generate(idx, 10, temperature=0.0, return_logits=True, num_draft_tokens=3, spec_stats=stats, **kw)
        assert torch.equal(out, plain) and torch.equal(lg, lp)
        steps, acc = D.spec_trace_reference(plain, kw.get("prompt_lens", [9, 9]), 10, 3, 3, kw.get("eos_token_id"))
        assert stats["model_steps"] == steps and torch.equal(stats["accepted"], acc.sum(0))


def test_the_repeating_model_repeats():
    """What the GPU test of full acceptance relies on, on the fp32 twin: greedy repeats the prompt's last token."""
    g = SC.repeating_model("cpu", torch.float32)
    out = g.generate(SC.REPEAT_PROMPT, SC.REPEAT_NEW, temperature=0.0)
    assert (out[0, SC.REPEAT_PROMPT.shape[1]:] == SC.REPEAT_PROMPT[0, -1]).all()
    for K in (1, 3, 7):
        steps, acc = D.spec_trace_reference(out, [SC.REPEAT_PROMPT.shape[1]], SC.REPEAT_NEW, K)
        assert steps == -(-(SC.REPEAT_NEW - 1) // (K + 1)) and (acc[:-1] == K).all()


@pytest.mark.parametrize("kw", [dict(temperature=1.0), dict(top_k=5), dict(top_p=0.9), dict(repetition_penalty=1.2),
                                dict(no_repeat_ngram_size=2), dict(num_beams=2)], ids=lambda kw: next(iter(kw)))
def test_what_does_not_combine(kw):
    g = build_gpt2(SC.tiny_cfg(), seed=1, device="cpu", dtype=torch.float32)
    kw = dict(dict(temperature=0.0), **kw)
    with pytest.raises(ValueError, match="num_draft_tokens"):
        g.generate(torch.zeros(1, 4, dtype=torch.int64), 4, num_draft_tokens=2, **kw)
    for bad in (dict(num_draft_tokens=-1), dict(num_draft_tokens=2, draft_ngram=9), dict(num_draft_tokens=1.5)):
        with pytest.raises(ValueError):
            g.generate(torch.zeros(1, 4, dtype=torch.int64), 4, temperature=0.0, **bad)
