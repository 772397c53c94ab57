"""Beam search on the CPU: ``beam_step_reference`` against a brute-force sort, ``GPT.generate(num_beams=)`` against
exhaustive search and against its own equivalences, the input conditions of the GPU tests on the very tensors they
use, ``decode_attention(beam_table=)`` against a gathered cache, and the errors."""
import itertools
import math

import numpy as np
import pytest
import torch

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import DeviceRNG
from pytorch_distributed_example_amd.ops import decode as D

import beam_cases as BC


# --------------------------------------------------------------------------------------- the step's definition
def _brute_force(logits, V, K, S, fin, eos, first):
    """All ``K * V`` candidates of every group, written as loops, sorted by (score descending, flat index)."""
    x = logits.double()[:, :V]
    R = x.shape[0]
    res = []
    for b in range(R // K):
        cand = []
        for k in range(1 if first else K):
            r = b * K + k
            if fin[r]:
                cand.append((-float(S[r]), k * V + eos))
                continue
            m = x[r].max()
            lse = float(m + torch.log(torch.exp(x[r] - m).sum()))
            for v in range(V):
                cand.append((-(float(S[r]) + (float(x[r, v]) - lse)), k * V + v))
        cand.sort()
        res.append([(f // V, f % V, -s) for s, f in cand[:K + 1]])
    return res


@pytest.mark.parametrize("B,K,V,Vp,first", [(2, 3, 50, 56, False), (1, 4, 33, 40, False), (2, 3, 50, 56, True),
                                            (1, 1, 9, 16, False)])
def test_reference_matches_brute_force(B, K, V, Vp, first):
    g = torch.Generator().manual_seed(B * 100 + K * 10 + V)
    logits = (torch.randn(B * K, Vp, generator=g) * 3).to(torch.bfloat16)
    logits[0, 3] = logits[0, 5] = logits[0, :V].max()             # a tie at the top of row 0
    logits[:, V:] = 100.0                                          # pad columns never participate
    S = -(torch.rand(B * K, generator=g) * 4)
    fin = torch.arange(B * K) % 3 == 1
    parent, tok, score, info = D.beam_step_reference(logits, V, K, S, fin, 2, first=first, return_info=True)
    want = _brute_force(logits, V, K, S.double(), fin, 2, first)
    for b in range(B):
        assert [(int(parent[b, j]), int(tok[b, j])) for j in range(K)] == [(k, v) for k, v, _ in want[b][:K]]
        assert np.allclose(score[b].numpy(), [s for _, _, s in want[b][:K]], rtol=0, atol=1e-12)
        assert np.allclose(info["best"][b], [s for _, _, s in want[b]], rtol=0, atol=1e-12)
        diffs = [want[b][j][2] - want[b][j + 1][2] for j in range(K)
                 if not (want[b][j][0] == want[b][j + 1][0] and not fin[b * K + want[b][j][0]]
                         and logits[b * K + want[b][j][0], want[b][j][1]] == logits[b * K + want[b][j][0], want[b][j + 1][1]])]
        assert math.isclose(info["gap"][b], min(diffs, default=math.inf), rel_tol=0, abs_tol=1e-12)
    if K == 1:
        assert info["gap"][0] == math.inf          # the two best are row 0's tied maxima: resolved by index
    else:
        assert (info["gap"] < math.inf).all()
    # without an eos nothing is frozen
    p2, t2, _ = D.beam_step_reference(logits, V, K, S, fin, None, first=first)
    w2 = _brute_force(logits, V, K, S.double(), torch.zeros_like(fin), -1, first)
    assert [(int(p2[0, j]), int(t2[0, j])) for j in range(K)] == [(k, v) for k, v, _ in w2[0][:K]]


def test_gpu_kernel_test_input_conditions():
    """No kernel input of the GPU test has a gap below ``MIN_GAP``, scores stay below 64 in magnitude: the GPU
    comparison is exact for every case."""
    smallest = math.inf
    for shape in BC.KERNEL_SHAPES:
        for i in range(BC.N_KERNEL_INPUTS):
            _, _, score, info = BC.kernel_reference(i, *shape)
            smallest = min(smallest, float(info["gap"].min()))
            assert float(np.abs(info["best"][np.isfinite(info["best"])]).max()) < 64
    print(f"smallest gap over the {len(BC.KERNEL_SHAPES) * BC.N_KERNEL_INPUTS} kernel inputs: {smallest:.3e}")
    assert smallest >= BC.MIN_GAP


def test_hand_made_steps():
    cases = BC.hand_cases()
    ref = {name: BC.hand_reference(c) for name, c in cases.items()}
    p, t, s, _ = ref["all_equal"]
    assert p.tolist() == [[0, 0, 0, 0]] and t.tolist() == [[0, 1, 2, 3]]
    p, t, s, _ = ref["step0"]
    assert p.tolist() == [[0, 0, 0], [0, 0, 0]] and (t < 1000).all() and (s < 0).all()
    lg = cases["step0"]["logits"].float()[:, :1000]
    assert t[0].tolist() == lg[0].topk(3).indices.tolist() and t[1].tolist() == lg[3].topk(3).indices.tolist()
    p, t, s, _ = ref["all_finished"]
    assert p.tolist() == [[1, 2, 0, 3]] and (t == BC.EOS).all() and s.tolist() == [[-1.0, -2.0, -3.0, -4.0]]
    p, t, s, _ = ref["cross_beam_tie"]
    assert p.tolist() == [[0, 1]] and t[0, 0] == t[0, 1] and s[0, 0] == s[0, 1]
    p, t, s, _ = ref["chooses_eos"]
    assert (int(p[0, 0]), int(t[0, 0])) == (0, BC.EOS) and (int(p[0, 1]), int(t[0, 1])) == (1, BC.EOS)
    assert float(s[0, 1]) == -0.75


# --------------------------------------------------------------------------------------- generate on the CPU
def _small(V=16, seed=0, scale=4.0):
    m = build_gpt2(GPTConfig(block_size=32, vocab_size=V, padded_vocab=V, n_layer=1, n_head=1, n_embd=64), seed=seed,
                   dtype=torch.float32).eval()
    with torch.no_grad():
        m.transformer.ln_f.weight.fill_(scale)
    return m


@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
def test_exhaustive_search(length_penalty):
    """``K = 16`` beams over two steps of a 16-token vocabulary: step 0 prunes nothing (``K = V``), so step 1 sees all
    256 continuations and the 16 ranked hypotheses are the best 16 of them by summed fp64 log-probability.  (The
    definition needs ``K <= V`` at step 0, so a vocabulary of 4 cannot carry 16 beams.)"""
    m, V, K = _small(), 16, 16
    idx = torch.tensor([[3, 1, 4]])
    out, scores = m.generate(idx, 2, num_beams=K, length_penalty=length_penalty, return_beams=True)
    assert out.shape == (1, K, 5) and scores.shape == (1, K) and scores.dtype == torch.float32
    allc = []
    with torch.no_grad():
        for a, b in itertools.product(range(V), range(V)):
            lp = torch.log_softmax(m(torch.tensor([[3, 1, 4, a]])).double()[0, :, :V], -1)
            allc.append((-float(lp[2, a] + lp[3, b]) / 2.0 ** length_penalty, a * V + b))
    allc.sort()
    assert [(int(r[3]), int(r[4])) for r in out[0]] == [(f // V, f % V) for _, f in allc[:K]]
    assert (out[0, :, :3] == idx).all()
    assert np.allclose(scores[0].double().numpy(), [-s for s, _ in allc[:K]], rtol=1e-6, atol=1e-6)


def test_one_beam_is_greedy_and_the_default_call():
    m = _small(V=40)
    idx = torch.randint(0, 40, (3, 5), generator=torch.Generator().manual_seed(1))
    assert torch.equal(m.generate(idx, 8, num_beams=1, temperature=0.0), m.generate(idx, 8, temperature=0.0))
    assert torch.equal(m.generate(idx, 8, num_beams=1, seed=5, top_k=9), m.generate(idx, 8, seed=5, top_k=9))
    # K = 1 through the beam definition itself: the greedy tokens
    g = m.generate(idx, 8, temperature=0.0, return_logits=True)[1]
    S, fin, toks = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.bool), []
    for s in range(8):
        p, t, S = D.beam_step_reference(g[:, s], 40, 1, S, fin, None, first=s == 0)
        toks.append(t.reshape(3))
        S = S.reshape(3)
    assert torch.equal(torch.stack(toks, 1), m.generate(idx, 8, temperature=0.0)[:, 5:])
    # a generator is left alone
    gen = DeviceRNG(3)
    m.generate(idx, 4, num_beams=1, generator=gen)
    assert gen.draw_number() == 4


def test_ragged_batch_equals_each_prompt_alone():
    m = _small(V=40)
    lens = [4, 1, 6]
    idx = torch.randint(0, 40, (3, 7), generator=torch.Generator().manual_seed(2))
    out, sc, lg = m.generate(idx, 5, num_beams=3, prompt_lens=lens, pad_token_id=9, return_beams=True,
                             return_logits=True, eos_token_id=11)
    assert out.shape == (3, 3, 12) and lg.shape == (9, 5, 40)
    best = m.generate(idx, 5, num_beams=3, prompt_lens=lens, pad_token_id=9, eos_token_id=11)
    assert torch.equal(best, out[:, 0])
    for b, n in enumerate(lens):
        o1, s1, l1 = m.generate(idx[b:b + 1, :n], 5, num_beams=3, return_beams=True, return_logits=True,
                                eos_token_id=11)
        assert torch.equal(out[b, :, :n + 5], o1[0]) and (out[b, :, n + 5:] == 9).all()
        assert torch.allclose(sc[b], s1[0], rtol=0, atol=1e-6)
        assert torch.allclose(lg[3 * b:3 * b + 3], l1, rtol=0, atol=1e-5)
        assert (lg[3 * b + 1:3 * b + 3, 0] == 0).all()             # step 0 fills row b * K only


def test_final_ranking_and_eos_freezing():
    m = _small(V=40, scale=2.0)
    idx = torch.randint(0, 40, (2, 4), generator=torch.Generator().manual_seed(3))
    K, n_new = 4, 6
    free = m.generate(idx, n_new, num_beams=K, return_beams=True)[0]
    eos = int(free[0, 1, 4 + 1])                                   # the second token of a surviving hypothesis
    for lp in (0.0, 1.0, 2.0):
        tr = {}
        out, sc = m.generate(idx, n_new, num_beams=K, length_penalty=lp, eos_token_id=eos, return_beams=True,
                             _beam_trace=tr)
        assert tr["finished"].any() and (tr["len"][tr["finished"]] < n_new).any(), "no beam finished early"
        assert ((tr["len"] == n_new) | tr["finished"]).all()
        order, ranked = D.beam_rank_reference(tr["S"], tr["len"], K, lp)
        assert np.allclose(sc.double().numpy(), ranked.numpy(), rtol=1e-6, atol=1e-6)
        assert (np.diff(ranked.numpy(), axis=1) <= 0).all()
        want = (tr["S"].reshape(2, K) / tr["len"].reshape(2, K).double() ** lp)
        assert torch.equal(torch.gather(want, 1, order), ranked)
        for b in range(2):
            for i in range(K):
                gen = out[b, i, 4:].tolist()
                r = b * K + int(order[b, i])
                n = int(tr["len"][r])
                assert (eos in gen) == bool(tr["finished"][r])
                if eos in gen:                                     # frozen: eos repeated, len counts the first one
                    assert gen.index(eos) + 1 == n and all(t == eos for t in gen[n - 1:])


def test_twin_generation_gaps():
    """The prompts of the GPU tests: the fp32 twin's own beam search has no step closer than ``MIN_GAP``."""
    m = BC.twin()
    for B, K, T0, n_new, seed in BC.HYP_CASES:
        g = BC.step_gaps(m, BC.prompt(B, T0, seed), n_new, K)
        print(f"(B, K, T0, n_new) = {(B, K, T0, n_new)}: smallest gap {float(g.min()):.3e}")
        assert g.shape == (n_new, B) and float(g.min()) >= BC.MIN_GAP
    g = BC.step_gaps(m, BC.prompt(3, max(BC.RAGGED_LENS), BC.RAGGED_SEED), BC.RAGGED_NEW, BC.RAGGED_K,
                     prompt_lens=BC.RAGGED_LENS)
    assert float(g.min()) >= BC.MIN_GAP


# --------------------------------------------------------------------------------------- attention through the table
def test_decode_attention_with_table_equals_gathered_cache():
    class Cfg:
        n_layer, n_head, n_embd = 1, 2, 128

    B, K, H, Tmax = 2, 3, 2, 40
    R = B * K
    g = torch.Generator().manual_seed(8)
    for p, step in ((0, 0), (1, 1), (17, 2), (39, 3)):
        cache = D.KVCache(Cfg, R, Tmax, dtype=torch.float32)
        cache.data.copy_(torch.randn(cache.data.shape, generator=g))
        table = D.beam_table(B, K, Tmax)
        assert table.shape == (2, 16, 48) and table.dtype == torch.uint8
        assert table[:, :R, 0].tolist() == [[0, 0, 0, 3, 3, 3]] * 2
        grp = (torch.arange(R) // K * K)[:, None]
        table[step & 1, :R, :p] = (grp + torch.randint(0, K, (R, p), generator=g)).to(torch.uint8)
        table[(step & 1) ^ 1, :R] = (grp + torch.randint(0, K, (R, 48), generator=g)).to(torch.uint8)
        gathered = D.KVCache(Cfg, R, Tmax, dtype=torch.float32)
        gathered.data.copy_(cache.data)
        t = torch.arange(p)
        for r in range(R):
            gathered.data[0, :, r, :, :p] = cache.data[0, :, table[step & 1, r, :p].long(), :, t].permute(1, 2, 0, 3)
        qkv = torch.randn(R, 3 * H * 64, generator=g)
        state = D.DecodeState(pos=p, step=step)
        before = cache.data.clone()
        y = D.decode_attention(qkv, cache, 0, state, beam_table=table)
        assert torch.equal(y, D.decode_attention(qkv, gathered, 0, state))
        # row p of the row itself holds the new K and V; nothing else changed
        before[0, 0, :, :, p] = qkv[:, H * 64:2 * H * 64].reshape(R, H, 64)
        before[0, 1, :, :, p] = qkv[:, 2 * H * 64:].reshape(R, H, 64)
        assert torch.equal(cache.data, before)


# --------------------------------------------------------------------------------------- errors
def test_errors():
    m = _small(V=8)
    idx = torch.tensor([[1, 2, 3]])
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_beams"):
            m.generate(idx, 2, num_beams=bad)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(idx, 2, num_beams=9)                            # K > V
    m.generate(idx, 2, num_beams=8)
    for lp in (math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError, match="length_penalty"):
            m.generate(idx, 2, num_beams=2, length_penalty=lp)
    with pytest.raises(ValueError, match="return_beams"):
        m.generate(idx, 2, return_beams=True)
    off = dict(temperature=0.0, top_k=3, top_p=0.9, seed=1, generator=DeviceRNG(1), repetition_penalty=1.2,
               frequency_penalty=0.1, presence_penalty=0.1, logit_bias=torch.zeros(8), suppress_tokens=[1],
               min_new_tokens=1, no_repeat_ngram_size=2, bad_words_ids=[[1, 2]], stop_sequences=[[1, 2]])
    for name, value in off.items():
        with pytest.raises(ValueError, match=name):
            m.generate(idx, 2, num_beams=2, eos_token_id=5, **{name: value})
    with pytest.raises(ValueError):
        m.generate(idx, 2, num_beams=2, eos_token_id=8)
    # the CPU path has no 16-row limit
    big = _small(V=40)
    out = big.generate(torch.randint(0, 40, (3, 4), generator=torch.Generator().manual_seed(0)), 2, num_beams=6)
    assert out.shape == (3, 6)
    with pytest.raises(NotImplementedError):
        D.beam_table(3, 6, 16)
