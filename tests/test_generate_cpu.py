"""GPT-2 generation on the CPU: the sampling definition (``sample_reference``) and ``GPT.generate``
on an fp32 model -- the definition the GPU path is tested against."""
import numpy as np
import pytest
import torch

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import DeviceRNG, sample_reference
from pytorch_distributed_example_amd.ops.rng import snapshot_words


def _snap(seed, draw=0):
    r = DeviceRNG(seed)
    for _ in range(draw):
        r.next()
    return r.next()


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_sample_reference_distribution(temperature):
    """20 000 rows with the same logits: every token's frequency within 4 standard deviations of
    softmax(logits / T)."""
    n, V = 20000, 8
    torch.manual_seed(0)
    row = torch.randn(V) * 1.5
    tok = sample_reference(row.repeat(n, 1), V, _snap(1234), temperature).numpy()
    p = torch.softmax(row.double() * float(np.float32(1.0 / temperature)), 0).numpy()
    freq = np.bincount(tok, minlength=V) / n
    sd = np.sqrt(p * (1 - p) / n)
    assert (np.abs(freq - p) <= 4 * sd).all(), (freq, p, sd)


def test_top_k_one_is_greedy():
    torch.manual_seed(1)
    lg = torch.randn(64, 40) * 3
    greedy = sample_reference(lg, 37, _snap(5), 0.0)
    assert torch.equal(sample_reference(lg, 37, _snap(5), 1.0, top_k=1), greedy)
    assert torch.equal(greedy, lg[:, :37].argmax(1))


def test_top_k_candidates_and_ties():
    torch.manual_seed(2)
    n, V = 4000, 16
    row = torch.randn(V)
    row[[3, 9]] = row.max() + 1.0           # two equal maxima
    row[[1, 5, 12]] = row.max() - 0.5       # the 3rd largest value occurs three times
    allowed = {3, 9, 1, 5, 12}              # tie-inclusive: 5 candidates for top_k = 3
    tok, info = sample_reference(row.repeat(n, 1), V, _snap(7), 1.0, top_k=3, return_info=True)
    assert (info["ncand"] == 5).all() and (info["threshold"] == float(row[1])).all()
    seen = set(tok.tolist())
    assert seen <= allowed
    assert seen == allowed, "every tied token is a candidate and is drawn in 4000 rows"


def test_greedy_lowest_index_on_ties():
    lg = torch.zeros(3, 16)
    lg[1, [4, 11]] = 2.0
    lg[2, 15] = 5.0                          # column >= V: never participates
    assert sample_reference(lg, 12, _snap(0), 0.0).tolist() == [0, 4, 0]


def _tiny(seed=0):
    cfg = GPTConfig(block_size=512, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128)
    return build_gpt2(cfg, seed=seed, dtype=torch.float32)


@pytest.fixture(scope="module")
def model():
    return _tiny()


def _prompt(B=3, T0=5):
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 1000, (B, T0), generator=g)


def test_generate_shape_prompt_and_greedy(model):
    idx = _prompt()
    out, logits = model.generate(idx, 6, temperature=0.0, return_logits=True)
    assert out.shape == (3, 11) and out.dtype == torch.int64 and logits.shape == (3, 6, 1000)
    assert torch.equal(out[:, :5], idx)
    seq = idx
    with torch.no_grad():
        for _ in range(6):
            seq = torch.cat([seq, model(seq)[:, -1].argmax(-1, keepdim=True)], dim=1)
    assert torch.equal(out, seq)


def test_generate_seeds(model):
    idx = _prompt()
    a = model.generate(idx, 8, temperature=1.0, seed=3)
    assert torch.equal(a, model.generate(idx, 8, temperature=1.0, seed=3))
    assert not torch.equal(a, model.generate(idx, 8, temperature=1.0, seed=4))


def test_generate_generator_advances_and_reloads(model):
    idx = _prompt()
    gen = DeviceRNG(21)
    first = model.generate(idx, 4, generator=gen)
    assert gen.draw_number() == 4
    sd = gen.state_dict()
    cont = model.generate(first, 5, generator=gen)
    assert gen.draw_number() == 9
    gen2 = DeviceRNG(0)
    gen2.load_state_dict(sd)
    assert torch.equal(model.generate(first, 5, generator=gen2), cont)
    # one generator over 4 + 5 tokens draws what one call over 9 tokens draws
    assert torch.equal(model.generate(idx, 9, generator=DeviceRNG(21)), cont)


def test_generate_eos(model):
    idx = _prompt()
    free = model.generate(idx, 8, temperature=1.0, seed=5)
    eos = int(free[0, 5 + 2])                # the third token row 0 generates
    first = (free[0, 5:] == eos).nonzero()[0, 0].item()
    out = model.generate(idx, 8, temperature=1.0, seed=5, eos_token_id=eos)
    assert torch.equal(out[0, :5 + first + 1], free[0, :5 + first + 1])
    assert (out[0, 5 + first:] == eos).all()
    for b in (1, 2):
        hit = (free[b, 5:] == eos).nonzero()
        stop = 5 + (hit[0, 0].item() if len(hit) else 8)
        assert torch.equal(out[b, :stop], free[b, :stop])


def test_generate_limits_and_side_effects(model):
    idx = _prompt()
    with pytest.raises(ValueError):
        model.generate(idx, 512 - 5 + 1)
    model.seed_dropout(9)
    draw = model.rng.draw_number()
    for training in (True, False):
        model.train(training)
        model.generate(idx, 2, seed=0)
        assert model.training is training
    model.eval()
    assert model.rng.draw_number() == draw


def test_cached_decode_ops_match_full_forward(model):
    """The CPU definitions of the decode ops (cache fill, decode embedding / attention, skinny linear,
    sampler bookkeeping on a DecodeState) chained as the GPU decode step chains them: every step's logits
    equal a full forward over the tokens so far."""
    from pytorch_distributed_example_amd.ops import decode as D
    from pytorch_distributed_example_amd.ops import transformer as T

    cfg, t = model.config, model.transformer
    B, T0, n = 2, 7, 4
    idx = _prompt(B, T0)
    wte, wpe = t.wte.weight, t.wpe.weight
    with torch.no_grad():
        cache = D.KVCache(cfg, B, T0 + n, dtype=torch.float32)
        x, delta = T.embedding(idx, wte, wpe), None
        for l, blk in enumerate(t.h):
            x, delta, qkv = blk.forward_deferred_qkv(x, delta)
            D.cache_fill(qkv, cache, l, T0)
        h = T.add_layer_norm_residual(x[:, -1], delta[:, -1], t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
        state = D.DecodeState(None, DeviceRNG(3).state, pos=T0 - 1, step=0)
        out = torch.zeros(B, T0 + n, dtype=torch.int64)
        out[:, :T0] = idx
        nxt = torch.zeros(B, dtype=torch.int64)
        kept = torch.zeros(B, n, cfg.vocab_size)
        for i in range(n):
            if i:
                x, delta = D.decode_embed(nxt, wte, wpe, state), None
                for blk in t.h:
                    x, delta = blk.decode_deferred(x, delta, cache, state)
                h = T.add_layer_norm_residual(x, delta, t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
            D.sample(D.skinny_linear(h, wte), cfg.vocab_size, state, 1.0, 20, next=nxt, out=out, logits_out=kept,
                     T0=T0)
            assert state.pos() == T0 + i and state.step() == i + 1
            ref = model(out[:, :T0 + i])[:, -1]
            assert torch.allclose(kept[:, i], ref, atol=1e-5, rtol=1e-4), i
            assert torch.equal(out[:, T0 + i], nxt)
        assert snapshot_words(state.rng)[2] == n      # one draw number per token
