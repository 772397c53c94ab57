"""GPT-2 generation on the GPU: the decode kernels against fp32 / numpy references, and
``GPT.generate`` against a teacher-forced CPU fp32 twin."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import DeviceRNG, sample_reference
from pytorch_distributed_example_amd.ops import decode as D

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16


def rel_err(a, b):      # tests/test_transformer_gpu.py's definition
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


# --------------------------------------------------------------------------------------- skinny linear
@pytest.mark.parametrize("K,N", [(64, 24), (128, 384), (768, 2304), (3072, 768), (128, 1024)])
@pytest.mark.parametrize("M", [1, 3, 16])
def test_skinny_linear(M, K, N):
    g = torch.Generator().manual_seed(M * 7 + K + N)
    x = torch.randn(M, K, generator=g).to(dev, BF16)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev, BF16)
    b = (0.5 * torch.randn(N, generator=g)).to(dev, BF16)
    for bias, gelu, bound in ((b, False, 1e-2), (b, True, 2e-2), (None, False, 1e-2)):
        y = D.skinny_linear(x, w, bias, gelu=gelu)
        ref = F.linear(x.float(), w.float(), None if bias is None else bias.float())
        if gelu:
            ref = F.gelu(ref, approximate="tanh")
        assert y.shape == (M, N) and y.dtype == BF16
        e = rel_err(y, ref)
        assert e < bound, (bias is not None, gelu, e)
        assert torch.equal(y, D.skinny_linear(x, w, bias, gelu=gelu))


def test_skinny_linear_rejects_unsupported_shapes():
    def call(M, K, N):
        return D.skinny_linear(torch.zeros(M, K, device=dev, dtype=BF16), torch.zeros(N, K, device=dev, dtype=BF16))

    call(16, 64, 8)
    for M, K, N in ((17, 64, 8), (4, 40, 8), (4, 64, 12)):
        with pytest.raises(NotImplementedError):
            call(M, K, N)
    with pytest.raises(NotImplementedError):
        D.skinny_linear(torch.zeros(2, 64, device=dev), torch.zeros(8, 64, device=dev))


# --------------------------------------------------------------------------------------- decode attention
class _Cfg:
    n_layer, n_head, n_embd = 1, 2, 128


def _random_cache(B, Tmax, seed=0):
    cache = D.KVCache(_Cfg, B, Tmax, dev)
    g = torch.Generator().manual_seed(seed)
    cache.data.copy_(torch.randn(cache.data.shape, generator=g).to(BF16))
    return cache


def _attn_one_query_ref(qkv_row, K, V, H):
    """``_attn_ref``'s arithmetic (tests/test_transformer_gpu.py) for one query over keys [B, H, n, 64]."""
    B = qkv_row.shape[0]
    q = qkv_row.float()[:, :H * 64].reshape(B, H, 1, 64)
    s = (q @ K.float().transpose(-1, -2)) / math.sqrt(64)
    return (torch.softmax(s, -1) @ V.float()).reshape(B, H * 64)


@pytest.mark.parametrize("B", [1, 3])
def test_decode_attention(B):
    H, Tmax = 2, 512
    cache = _random_cache(B, Tmax)
    before = cache.data.clone()
    g = torch.Generator().manual_seed(B)
    for p in (0, 1, 127, 128, 129, 255, 256, 511):
        qkv = torch.randn(B, 3 * H * 64, generator=g).to(dev, BF16)
        state = D.DecodeState(dev, pos=p)
        y = D.decode_attention(qkv, cache, 0, state)
        kn, vn = (qkv[:, s * H * 64:(s + 1) * H * 64].reshape(B, H, 1, 64) for s in (1, 2))
        ref = _attn_one_query_ref(qkv, torch.cat([before[0, 0, :, :, :p], kn], 2),
                                  torch.cat([before[0, 1, :, :, :p], vn], 2), H)
        e = rel_err(y, ref)
        assert e < 2e-2, (p, e)
        # row p holds the new K and V bit for bit; nothing else changed
        assert torch.equal(cache.data[0, 0, :, :, p], kn[:, :, 0]) and torch.equal(cache.data[0, 1, :, :, p], vn[:, :, 0])
        expect = before.clone()
        expect[0, 0, :, :, p], expect[0, 1, :, :, p] = kn[:, :, 0], vn[:, :, 0]
        assert torch.equal(cache.data, expect), p
        # a second run on the restored cache is bit-identical
        cache.data.copy_(before)
        assert torch.equal(D.decode_attention(qkv, cache, 0, state), y), p
        cache.data.copy_(before)
        assert state.pos() == p           # attention reads the state, only the sampler advances it


def test_decode_attention_independent_of_cache_length():
    B, H, p = 2, 2, 200
    big = _random_cache(B, 512, seed=3)
    small = D.KVCache(_Cfg, B, 256, dev)
    small.data.copy_(big.data[:, :, :, :, :256])
    qkv = torch.randn(B, 3 * H * 64, generator=torch.Generator().manual_seed(9)).to(dev, BF16)
    state = D.DecodeState(dev, pos=p)
    assert torch.equal(D.decode_attention(qkv, big, 0, state), D.decode_attention(qkv, small, 0, state))


# --------------------------------------------------------------------------------------- sampler
SETTINGS = [(t, k) for t in (0.0, 0.7, 1.0) for k in (None, 1, 50)]


def sampler_logits(B, V, Vp):
    """randn * 3 in bf16; with B >= 3 row 1 is all-equal and row 2's maximum occurs twice."""
    g = torch.Generator().manual_seed(1000 + B + V)
    lg = (torch.randn(B, Vp, generator=g) * 3).to(BF16)
    if B >= 3:
        lg[1] = 0.75
        top = int(lg[2, :V].argmax())
        lg[2, V - 3 if top != V - 3 else 5] = lg[2, top]
    return lg


def sampler_seed(B, V, i):
    return 77 + 1000 * i + 10 * B + V


@pytest.mark.parametrize("V,Vp", [(1000, 1024), (50257, 50304)])
@pytest.mark.parametrize("B", [1, 5, 16])
def test_sampler_matches_reference(B, V, Vp):
    lg = sampler_logits(B, V, Vp)
    lgd = lg.to(dev)
    for i, (t, k) in enumerate(SETTINGS):
        snap = DeviceRNG(sampler_seed(B, V, i)).next()
        ref, info = sample_reference(lg, V, snap, t, k, return_info=True)
        thr = torch.full((B,), -1, device=dev, dtype=torch.int32)
        tok = D.sample(lgd, V, snap.to(dev), t, k, threshold_out=thr).cpu()
        assert (D.key16_to_float(thr) == info["threshold"]).all(), (t, k)        # exact
        if t == 0:
            assert torch.equal(tok, ref), (t, k)
            continue
        # a sampled token may differ only where the reference's own fp64 gap between best and runner-up is
        # below 1e-4 (fp32 score sum good to 4e-6, two logf under 1e-5: a factor of ten); the seeds are
        # chosen so that no row is that close, which makes the comparison exact
        close = info["gap"] < 1e-4
        assert not close.any(), (t, k, info["gap"].min())
        differ = (tok != ref).numpy()
        assert not (differ & ~close).any() and differ.sum() <= 1, (t, k, tok, ref)


def test_sampler_side_effects_two_calls():
    B, V, Vp, T0, n_new = 5, 1000, 1024, 4, 3
    g = torch.Generator().manual_seed(5)
    lgs = [(torch.randn(B, Vp, generator=g) * 3).to(BF16) for _ in range(2)]
    rng = DeviceRNG(31)
    for _ in range(6):
        rng.next()                                       # a draw number other than 0
    state = D.DecodeState(dev, rng.state.to(dev), pos=9, step=0)
    nxt = torch.zeros(B, device=dev, dtype=torch.int64)
    out = torch.full((B, T0 + n_new), -1, device=dev, dtype=torch.int64)
    lout = torch.zeros(B, n_new, V, device=dev, dtype=BF16)
    ref0 = sample_reference(lgs[0], V, rng.next(), 0.9, 40)
    ref1 = sample_reference(lgs[1], V, rng.next(), 0.9, 40)
    eos = int(ref0[0])                                   # row 0 finishes at the first call
    assert eos not in ref0[1:].tolist() and eos not in ref1[1:].tolist()
    for lg in lgs:
        D.sample(lg.to(dev), V, state, 0.9, 40, eos, next=nxt, out=out, logits_out=lout, T0=T0)
    ref1[0] = eos
    assert torch.equal(out.cpu()[:, T0], ref0) and torch.equal(out.cpu()[:, T0 + 1], ref1)
    assert (out.cpu()[:, :T0] == -1).all() and (out.cpu()[:, T0 + 2:] == -1).all()
    assert torch.equal(nxt.cpu(), ref1)
    assert state.finished.cpu().tolist() == [1] + [0] * 15
    assert torch.equal(lout.cpu()[:, 0], lgs[0][:, :V]) and torch.equal(lout.cpu()[:, 1], lgs[1][:, :V])
    assert (lout.cpu()[:, 2] == 0).all()
    assert state.pos() == 11 and state.step() == 2
    assert torch.equal(state.rng.cpu(), rng.state)       # the same seed and stream, draw number + 2


# --------------------------------------------------------------------------------------- whole model
def _tiny_cfg():
    return GPTConfig(block_size=512, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128)


@pytest.fixture(scope="module")
def twins():
    """bf16 GPU model and an fp32 CPU twin with identical (bf16-representable) weights."""
    g = build_gpt2(_tiny_cfg(), seed=0, device=dev)
    c = build_gpt2(_tiny_cfg(), seed=0, dtype=torch.float32)
    with torch.no_grad():
        for pc, pg in zip(c.parameters(), g.parameters()):
            pc.copy_(pg.float())
    return g, c


def _prompt(T0, B=3):
    return torch.randint(0, 1000, (B, T0), generator=torch.Generator().manual_seed(T0))


def _teacher_forced_failures(g, c, T0, n_new, after_prefill=None):
    idx = _prompt(T0)
    out, lg = g.generate(idx.to(dev), n_new, temperature=0.0, return_logits=True, _after_prefill=after_prefill)
    out, lg = out.cpu(), lg.float().cpu()
    assert out.shape == (3, T0 + n_new) and lg.shape == (3, n_new, 1000) and torch.equal(out[:, :T0], idx)
    assert torch.equal(out[:, T0:], lg.argmax(-1)), "token != lowest-index argmax of the returned logits"
    with torch.no_grad():
        ref = c(out[:, :-1])                             # teacher forcing: the twin sees the generated tokens
    fails = []
    for s in range(n_new):
        a, b = lg[:, s].double().flatten(), ref[:, T0 - 1 + s].double().flatten()
        cs = F.cosine_similarity(a, b, dim=0).item()
        e = ((a - b).norm() / b.norm()).item()
        if not (cs >= 0.995 and e < 3e-2):
            fails.append(f"step {s}: cos {cs:.5f}, rel L2 err {e:.3e}")
    return fails


@pytest.mark.parametrize("T0,n_new", [(5, 4), (128, 3), (130, 3), (120, 140)])
def test_generate_matches_teacher_forced_twin(twins, T0, n_new):
    fails = _teacher_forced_failures(*twins, T0, n_new)
    assert not fails, fails


def test_generate_check_catches_a_zeroed_cache_row(twins):
    def zero_row(cache):
        cache.data[:, :, :, :, 2] = 0

    fails = _teacher_forced_failures(*twins, 5, 4, after_prefill=zero_row)
    assert fails, "a zeroed KV cache row went unnoticed"


def test_generate_graph_replay_equals_eager(twins):
    g, _ = twins
    idx = _prompt(7).to(dev)
    a, la = g.generate(idx, 12, temperature=0.0, return_logits=True)
    b, lb = g.generate(idx, 12, temperature=0.0, return_logits=True, use_graph=False)
    assert torch.equal(a, b) and torch.equal(la, lb)
    a = g.generate(idx, 12, temperature=0.8, top_k=40, seed=11)
    assert torch.equal(a, g.generate(idx, 12, temperature=0.8, top_k=40, seed=11, use_graph=False))


def test_generate_seeds_generator_eos_and_side_effects(twins):
    g, _ = twins
    idx = _prompt(6).to(dev)
    params = [p.detach().clone() for p in g.parameters()]
    g.seed_dropout(4)
    draw = g.rng.draw_number()
    g.train()
    gen = DeviceRNG(13, device=dev)
    free = g.generate(idx, 10, temperature=1.0, generator=gen)
    assert g.training
    g.eval()
    assert gen.draw_number() == 10
    assert torch.equal(free, g.generate(idx, 10, temperature=1.0, seed=13))
    assert not torch.equal(free, g.generate(idx, 10, temperature=1.0, seed=14))
    eos = int(free[0, 6])                                # the first token row 0 generates
    out = g.generate(idx, 10, temperature=1.0, seed=13, eos_token_id=eos)
    assert (out[0, 6:] == eos).all()
    for b in (1, 2):
        hit = (free[b, 6:] == eos).nonzero()
        stop = 6 + (int(hit[0, 0]) if len(hit) else 10)
        assert torch.equal(out[b, :stop], free[b, :stop])
    with pytest.raises(ValueError):
        g.generate(idx, 512 - 6 + 1)
    with pytest.raises(NotImplementedError):
        g.generate(_prompt(6, B=17).to(dev), 2)
    assert not g.training and g.rng.draw_number() == draw
    assert all(torch.equal(p, q) for p, q in zip(g.parameters(), params))
