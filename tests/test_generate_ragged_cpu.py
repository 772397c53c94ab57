"""Nucleus (top-p) sampling and ragged prompt batches on the CPU: the definition in ``sample_reference``,
the input conditions of the GPU sampler test, ``GPT.generate(prompt_lens=...)`` on an fp32 model and the
CPU definitions of the decode ops with per-row positions."""
import numpy as np
import pytest
import torch

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.ops import (DeviceRNG, LogitProcessors, TokenCounts, process_logits_reference,
                                                 sample_reference)
from pytorch_distributed_example_amd.ops.rng import snapshot_words

import generate_cases as GC


def _snap(seed):
    return DeviceRNG(seed).next()


# --------------------------------------------------------------------------------------- top-p definition
def test_top_p_hand_made_row():
    n, V = 4000, 16
    lg = GC.hand_row(n)
    tok, info = sample_reference(lg, V, _snap(3), 1.0, top_p=0.5, return_info=True)
    assert (info["ncand"] == 2).all() and set(tok.tolist()) == {0, 1}
    assert (info["threshold_p"] == float(lg[0, 1])).all() and (info["threshold"] == info["threshold_p"]).all()
    # 0.75 lies inside the tied pair of 0.1s (0.7 < 0.75 <= 0.9): both are kept
    tok, info = sample_reference(lg, V, _snap(4), 1.0, top_p=0.75, return_info=True)
    assert (info["ncand"] == 4).all() and (info["threshold"] == float(lg[0, 2])).all()
    assert set(tok.tolist()) == {0, 1, 2, 3}, "every kept token, the tied ones included, is drawn in 4000 rows"
    # the mass of a tiny nucleus: the top token alone
    tok, info = sample_reference(lg, V, _snap(5), 1.0, top_p=0.05, return_info=True)
    assert (info["ncand"] == 1).all() and (tok == 0).all()


def test_top_p_distribution():
    """20 000 equal rows: every frequency within 4 standard deviations of the renormalised nucleus."""
    n, V = 20000, 16
    tok = sample_reference(GC.hand_row(n), V, _snap(1234), 1.0, top_p=0.75).numpy()
    p = np.where(np.arange(V) < 4, GC.HAND_P, 0.0)
    p = p / p.sum()
    freq = np.bincount(tok, minlength=V) / n
    sd = np.sqrt(p * (1 - p) / n)
    assert (np.abs(freq - p) <= 4 * sd).all(), (freq, p, sd)


def test_top_p_with_temperature_uses_the_tempered_mass():
    # at T = 0.5 the probabilities are squared and renormalised: 0.16, 0.09, 0.01, 0.01, ... / 0.2727...
    lg = GC.hand_row(8)
    sq = GC.HAND_P ** 2 / (GC.HAND_P ** 2).sum()
    assert sq[0] < 0.6 < sq[0] + sq[1] < 0.93 < sq[:4].sum()
    assert (sample_reference(lg, 16, _snap(1), 0.5, top_p=0.6, return_info=True)[1]["ncand"] == 2).all()
    assert (sample_reference(lg, 16, _snap(1), 0.5, top_p=0.93, return_info=True)[1]["ncand"] == 4).all()


def test_top_p_equivalences():
    torch.manual_seed(5)
    lg = torch.randn(64, 40) * 3
    V = 37
    for k in (None, 7):
        base = sample_reference(lg, V, _snap(9), 0.8, k)
        assert torch.equal(sample_reference(lg, V, _snap(9), 0.8, k, top_p=None), base)
        assert torch.equal(sample_reference(lg, V, _snap(9), 0.8, k, top_p=1.0), base)
    greedy = sample_reference(lg, V, _snap(9), 0.0)
    assert torch.equal(sample_reference(lg, V, _snap(9), 0.0, top_p=0.5), greedy)
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            sample_reference(lg, V, _snap(9), 1.0, top_p=bad)
    # with top-k the mass is taken inside the top-k set: top-2 of the hand row is {0.4, 0.3}, and 0.6 of
    # its mass 0.7 is 0.42 > 0.4, so both stay; over all 16 columns 0.6 <= 0.7 keeps the same two, but 0.55
    # tells them apart: 0.55 * 0.7 = 0.385 <= 0.4 keeps one token, 0.55 of everything keeps two
    hr = GC.hand_row(4)
    assert (sample_reference(hr, 16, _snap(2), 1.0, 2, top_p=0.6, return_info=True)[1]["ncand"] == 2).all()
    assert (sample_reference(hr, 16, _snap(2), 1.0, 2, top_p=0.55, return_info=True)[1]["ncand"] == 1).all()
    assert (sample_reference(hr, 16, _snap(2), 1.0, None, top_p=0.55, return_info=True)[1]["ncand"] == 2).all()


def test_top_p_info_is_consistent_with_the_definition():
    torch.manual_seed(6)
    B, V, P, T, eps = 32, 200, 0.8, 0.9, 1e-3
    lg = (torch.randn(B, 208) * 2).bfloat16().float()
    tok, info = sample_reference(lg, V, _snap(8), T, 60, top_p=P, eps=eps, return_info=True)
    x = lg.double().numpy()[:, :V]
    inv_t = float(np.float32(1.0 / T))
    for b in range(B):
        kth = np.sort(x[b])[V - 60]
        cand = x[b] >= kth
        z = x[b] * inv_t
        w = np.where(cand, np.exp(z - z[cand].max()), 0.0)
        W = w.sum()
        tp = None
        for t in sorted(set(x[b][cand]), reverse=True):     # the definition, value by value
            if w[x[b] >= t].sum() >= P * W:
                tp = t
                break
        assert tp == info["threshold_p"][b] == info["threshold"][b] and tp >= kth
        slack = min(P * W - w[x[b] > tp].sum(), w[x[b] >= tp].sum() - P * W) / W
        assert slack >= 0 and abs(slack - info["p_slack"][b]) < 1e-12
        assert info["ncand"][b] == (x[b] >= tp).sum()
    lo, hi = info["threshold_p_bracket"]
    assert (lo <= info["threshold_p"]).all() and (info["threshold_p"] <= hi).all()
    assert (lo == sample_reference(lg, V, _snap(8), T, 60, top_p=P + eps, return_info=True)[1]["threshold_p"]).all()
    assert (hi == sample_reference(lg, V, _snap(8), T, 60, top_p=P - eps, return_info=True)[1]["threshold_p"]).all()
    # clamped into (0, 1]: the bracket of a mass near 1 ends at the smallest candidate, near 0 at the largest
    info1 = sample_reference(lg, V, _snap(8), T, 60, top_p=0.99995, return_info=True)[1]
    assert (info1["threshold_p_bracket"][0] == np.sort(x, axis=1)[:, V - 60]).all()
    info0 = sample_reference(lg, V, _snap(8), T, 60, top_p=5e-5, return_info=True)[1]
    assert (info0["threshold_p_bracket"][1] == x.max(axis=1)).all()
    # the reference's own threshold handed back reproduces token and candidates
    tok2, info2 = sample_reference(lg, V, _snap(8), T, None, _threshold=info["threshold"], return_info=True)
    assert torch.equal(tok, tok2) and (info2["ncand"] == info["ncand"]).all() and (info2["gap"] == info["gap"]).all()


def test_gpu_sampler_test_input_conditions():
    """The 528 (row, setting) cases of the GPU sampler test: at most 16 may have the target mass within
    1e-4 of a boundary between two thresholds (there the GPU test accepts the bracket instead of the exact
    threshold), and no row's best-versus-runner-up gap may be below 1e-4.  The count depends on the logits
    and settings only and is 7; the gaps depend on the seeds of ``generate_cases.topp_seed``."""
    close, total = 0, 0
    for B, V, Vp in GC.SAMPLER_SHAPES:
        lg = GC.sampler_logits(B, V, Vp)
        for i, (t, k, p) in enumerate(GC.TOPP_SETTINGS):
            _, info = sample_reference(lg, V, GC.topp_snapshot(B, V, i), t, k, top_p=p, return_info=True)
            close += int((info["p_slack"] < GC.P_SLACK).sum())
            total += B
            assert (info["gap"] >= GC.GAP).all(), (B, V, i, info["gap"].min())
            if B >= 3:
                assert info["ncand"][1] == V        # the all-equal row keeps everything
    assert total == GC.N_TOPP_CASES == 528
    print("cases with p_slack < 1e-4:", close)
    assert close <= GC.MAX_CLOSE_CASES, close


# --------------------------------------------------------------------------------------- ragged generate
@pytest.fixture(scope="module")
def model():
    return build_gpt2(GC.tiny_cfg(), seed=0, dtype=torch.float32)


LENS = (5, 1, 9)


def test_ragged_generate_layout_logits_and_greedy(model):
    n_new, pad = 6, 7
    idx = GC.ragged_prompt(LENS, width=11)
    gen = DeviceRNG(2)
    out, logits = model.generate(idx, n_new, temperature=0.0, return_logits=True, prompt_lens=list(LENS),
                                 pad_token_id=pad, generator=gen)
    assert out.shape == (3, 11 + n_new) and out.dtype == torch.int64 and logits.shape == (3, n_new, 1000)
    assert gen.draw_number() == n_new
    for b, n in enumerate(LENS):
        assert torch.equal(out[b, :n], idx[b, :n])
        assert (out[b, n + n_new:] == pad).all()
        seq = idx[b:b + 1, :n]
        with torch.no_grad():
            for s in range(n_new):                     # the row on its own, unpadded
                ref = model(seq)[:, -1]
                assert torch.allclose(logits[b:b + 1, s], ref, atol=1e-5, rtol=1e-4), (b, s)
                seq = torch.cat([seq, ref.argmax(-1, keepdim=True)], dim=1)
        assert torch.equal(out[b, :n + n_new], seq[0])
    # a tensor of lengths, and other junk past the prompts: the same result
    idx2 = idx.clone()
    for b, n in enumerate(LENS):
        idx2[b, n:] = 999
    out2 = model.generate(idx2, n_new, temperature=0.0, prompt_lens=torch.tensor(LENS), pad_token_id=pad)
    assert torch.equal(out, out2)


def test_ragged_generate_sampled_rows_and_eos(model):
    idx = GC.ragged_prompt(LENS)
    kw = dict(temperature=0.8, top_k=40, top_p=0.9, prompt_lens=list(LENS))
    free = model.generate(idx, 8, seed=5, **kw)
    assert torch.equal(free, model.generate(idx, 8, seed=5, **kw))
    assert not torch.equal(free, model.generate(idx, 8, seed=6, **kw))
    eos = int(free[1, LENS[1] + 2])                    # the third token row 1 generates
    out = model.generate(idx, 8, seed=5, eos_token_id=eos, **kw)
    for b, n in enumerate(LENS):
        hit = (free[b, n:n + 8] == eos).nonzero()
        stop = n + (hit[0, 0].item() if len(hit) else 8)
        assert torch.equal(out[b, :stop], free[b, :stop])
        assert (out[b, stop:n + 8] == eos).all() and (out[b, n + 8:] == 0).all()


def test_uniform_lengths_equal_the_call_without_them(model):
    idx = GC.ragged_prompt((6, 6, 6))
    for kw in (dict(temperature=0.0), dict(temperature=0.9, top_k=30, top_p=0.8, seed=4)):
        a, la = model.generate(idx, 5, return_logits=True, **kw)
        b, lb = model.generate(idx, 5, return_logits=True, prompt_lens=[6, 6, 6], **kw)
        assert torch.equal(a, b) and torch.equal(la, lb)
    a = model.generate(idx, 5, temperature=0.9, seed=4)
    assert torch.equal(a, model.generate(idx, 5, temperature=0.9, seed=4, top_p=1.0))
    assert torch.equal(a, model.generate(idx, 5, temperature=0.9, seed=4, top_p=None))


def test_ragged_generate_limits(model):
    idx = GC.ragged_prompt(LENS)
    for lens in ([5, 0, 9], [5, 1, 10], [5, 1], [5, 1, 9, 2]):
        with pytest.raises(ValueError):
            model.generate(idx, 2, prompt_lens=lens)
    wide = GC.ragged_prompt((5, 1, 500), width=510)
    model.generate(wide, 12, temperature=0.0, prompt_lens=[5, 1, 500])        # 500 + 12 == block_size
    with pytest.raises(ValueError):
        model.generate(wide, 13, prompt_lens=[5, 1, 500])
    for pad in (-1, 1000):
        with pytest.raises(ValueError):
            model.generate(idx, 2, prompt_lens=list(LENS), pad_token_id=pad)
    for p in (0.0, 1.01, -0.5):
        with pytest.raises(ValueError):
            model.generate(idx, 2, top_p=p)


def test_cached_decode_ops_with_row_offsets_match_full_forward(model):
    """``test_cached_decode_ops_match_full_forward`` with a ragged batch: the CPU definitions of the decode
    ops, chained as the GPU decode step chains them with per-row offsets in the state, give every row the
    logits of a full forward over that row's own tokens."""
    from pytorch_distributed_example_amd.ops import decode as D
    from pytorch_distributed_example_amd.ops import transformer as T

    cfg, t = model.config, model.transformer
    lens, n = [7, 2, 4], 4
    B, T0 = len(lens), max(lens)
    idx = GC.ragged_prompt(lens)
    ln = torch.tensor(lens)
    rows = torch.arange(B)
    wte, wpe = t.wte.weight, t.wpe.weight
    with torch.no_grad():
        cache = D.KVCache(cfg, B, T0 + n, dtype=torch.float32)
        x, delta = T.embedding(idx, wte, wpe), None
        for l, blk in enumerate(t.h):
            x, delta, qkv = blk.forward_deferred_qkv(x, delta)
            D.cache_fill(qkv, cache, l, T0)
        h = T.add_layer_norm_residual(x[rows, ln - 1], delta[rows, ln - 1], t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
        state = D.DecodeState(None, DeviceRNG(3).state, pos=T0 - 1, step=0, row_offsets=[m - T0 for m in lens])
        assert state.pos() == T0 - 1 and state.row_pos(B) == [m - 1 for m in lens]
        out = torch.full((B, T0 + n), -1, dtype=torch.int64)
        nxt = torch.zeros(B, dtype=torch.int64)
        kept = torch.zeros(B, n, cfg.vocab_size)
        for i in range(n):
            if i:
                x, delta = D.decode_embed(nxt, wte, wpe, state), None
                for blk in t.h:
                    x, delta = blk.decode_deferred(x, delta, cache, state)
                h = T.add_layer_norm_residual(x, delta, t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
            D.sample(D.skinny_linear(h, wte), cfg.vocab_size, state, 1.0, 20, next=nxt, out=out, logits_out=kept,
                     T0=T0, top_p=0.9)
            assert state.pos() == T0 + i and state.step() == i + 1
            for b, m in enumerate(lens):
                assert out[b, m + i] == nxt[b]
                seq = torch.cat([idx[b, :m], out[b, m:m + i]])[None]
                assert torch.allclose(kept[b:b + 1, i], model(seq)[:, -1], atol=1e-5, rtol=1e-4), (b, i)
        for b, m in enumerate(lens):                     # nothing outside the rows' own slots was written
            assert (out[b, :m] == -1).all() and (out[b, m + n:] == -1).all()
        assert snapshot_words(state.rng)[2] == n         # one draw number per token


# --------------------------------------------------------------------------------------- more rows than the GPU takes
def _reference_loop(model, idx, n_new, eos=None, procs=None, temperature=0.0, top_k=None, seed=0):
    """The definition, written out: one full forward per token over a batch of one prompt length, the choice by
    ``sample_reference`` (on ``process_logits_reference`` with processors), the counts and the eos rule by hand.
    Returns the ``[B, T0 + n_new]`` tokens and each row's step at which it became finished (-1: never)."""
    B, V = idx.shape[0], 1000
    seq, fin, fin_step = idx.clone(), torch.zeros(B, dtype=torch.bool), [-1] * B
    gen = DeviceRNG(seed)
    counts = torch.zeros(B, V, dtype=torch.int32)
    for b in range(B):
        counts[b, idx[b]] |= TokenCounts.PROMPT
    for s in range(n_new):
        with torch.no_grad():
            lg = model(seq)[:, -1]
        if procs is not None:
            lg = process_logits_reference(lg, V, counts, procs, s)
        tok = sample_reference(lg, V, gen.next(), temperature, top_k)
        if eos is not None:
            tok = torch.where(fin, torch.full_like(tok, eos), tok)
            for b in torch.nonzero(~fin & (tok == eos)).flatten().tolist():
                fin_step[b] = s
            fin = fin | (tok == eos)
        counts[torch.arange(B), tok] += 1
        seq = torch.cat([seq, tok[:, None]], dim=1)
    return seq, fin_step


@pytest.mark.parametrize("case", ["no_processors", "planted", "planted_frequency_penalty"])
def test_seventeen_rows_with_eos(model, case):
    """``B = 17`` on the CPU with an eos that a row past the 16 of the device state emits early, against the loop
    above.  ``planted``: a ``[B, V]`` ``logit_bias`` makes the greedy run emit it at once in rows 3 and 16.  A bias is
    itself a processor and the tiny model's free greedy run repeats one token per row, so ``no_processors`` is a
    sampled run whose eos is what row 16 of the free run emits at step 1, where the free run's later tokens differ
    from it: only the rule keeps the row emitting eos."""
    B, T0, n_new = 17, 3, 6
    idx = GC.ragged_prompt((T0,) * B)
    kw, sampling = {}, dict(temperature=0.0)
    if case == "no_processors":
        sampling = dict(temperature=0.9, top_k=30, seed=6)
        free, _ = _reference_loop(model, idx, n_new, **sampling)
        eos = int(free[16, T0 + 1])
        assert (free[16, T0 + 2:] != eos).any(), free[16]
    else:
        eos = 990
        bias = torch.zeros(B, 1000)
        bias[16, eos] = bias[3, eos] = 1e4
        kw = dict(logit_bias=bias, frequency_penalty=0.3 if case == "planted_frequency_penalty" else 0.0)
    want, fin_step = _reference_loop(model, idx, n_new, eos, LogitProcessors(eos_token_id=eos, **kw) if kw else None,
                                     **sampling)
    assert any(0 <= fin_step[b] < n_new - 1 for b in range(16, B)), fin_step     # or the test shows nothing
    assert any(s < 0 for s in fin_step), fin_step
    out = model.generate(idx, n_new, eos_token_id=eos, **sampling, **kw)
    assert torch.equal(out, want)
    for b, s in enumerate(fin_step):
        if s >= 0:
            assert (out[b, T0 + s:] == eos).all()
    # the sampled call, with and without a processor, runs too and keeps the rule
    for kw2 in ({}, dict(frequency_penalty=0.3)):
        smp = model.generate(idx, n_new, temperature=0.9, top_k=30, seed=4, eos_token_id=eos, **dict(kw, **kw2))
        for b in range(B):
            hit = torch.nonzero(smp[b, T0:] == eos).flatten()
            assert len(hit) == 0 or (smp[b, T0 + int(hit[0]):] == eos).all()


@pytest.mark.parametrize("lens", [None, list(LENS)], ids=["uniform", "ragged"])
@pytest.mark.parametrize("kw", [{}, dict(frequency_penalty=0.3), dict(no_repeat_ngram_size=2)],
                         ids=["plain", "processors", "constraints"])
def test_draw_number_advances_by_the_tokens_generated(model, lens, kw):
    idx = GC.ragged_prompt(LENS if lens else (6, 6, 6))
    gen = DeviceRNG(8)
    a = model.generate(idx, 5, temperature=0.9, top_k=30, generator=gen, prompt_lens=lens, **kw)
    assert gen.draw_number() == 5
    model.generate(idx, 3, temperature=0.9, top_k=30, generator=gen, prompt_lens=lens, **kw)
    assert gen.draw_number() == 8
    if lens is None and not kw:          # 5 + 3 tokens from one generator are the 8 of one call
        gen = DeviceRNG(8)
        first = model.generate(idx, 5, temperature=0.9, top_k=30, generator=gen)
        assert torch.equal(first, a)
        assert torch.equal(model.generate(first, 3, temperature=0.9, top_k=30, generator=gen),
                           model.generate(idx, 8, temperature=0.9, top_k=30, generator=DeviceRNG(8)))
