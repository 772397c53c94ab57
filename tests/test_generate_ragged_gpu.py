"""Ragged prompt batches and nucleus (top-p) sampling on the GPU: the decode kernels with per-row
positions against fp32 references and against their own uniform-position results (bit for bit), the
sampler's nucleus stage against ``sample_reference``, and ``GPT.generate(prompt_lens=...)`` against a
teacher-forced CPU fp32 twin, row by row."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.ops import DeviceRNG, sample_reference
from pytorch_distributed_example_amd.ops import decode as D

import generate_cases as GC
from test_generate_gpu import _attn_one_query_ref, _random_cache, rel_err

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16


def _state(positions, **kw):
    base = max(positions)
    return D.DecodeState(dev, pos=base, row_offsets=[p - base for p in positions], **kw)


# --------------------------------------------------------------------------------------- decode ops
@pytest.mark.parametrize("positions", [(0, 127, 300), (128, 129, 511), (255, 256, 1)])
def test_decode_attention_per_row_positions(positions):
    B, H, Tmax = 3, 2, 512
    cache = _random_cache(B, Tmax, seed=7)
    before = cache.data.clone()
    qkv = torch.randn(B, 3 * H * 64, generator=torch.Generator().manual_seed(sum(positions))).to(dev, BF16)
    state = _state(positions)
    words = state.buf.clone()
    assert state.pos() == max(positions) and state.row_pos(B) == list(positions)
    y = D.decode_attention(qkv, cache, 0, state)
    after = cache.data.clone()
    kn, vn = (qkv[:, s * H * 64:(s + 1) * H * 64].reshape(B, H, 64) for s in (1, 2))
    expect = before.clone()
    for b, p in enumerate(positions):
        ref = _attn_one_query_ref(qkv[b:b + 1], torch.cat([before[0, 0, b:b + 1, :, :p], kn[b:b + 1, :, None]], 2),
                                  torch.cat([before[0, 1, b:b + 1, :, :p], vn[b:b + 1, :, None]], 2), H)
        e = rel_err(y[b:b + 1], ref)
        print(f"positions {positions} row {b}: rel_err {e:.3e}")
        assert e < 2e-2, (positions, b, e)
        expect[0, 0, b, :, p], expect[0, 1, b, :, p] = kn[b], vn[b]
    # the cache changed at (b, p_b) only, and there it holds the new K / V bit for bit
    assert torch.equal(after, expect)
    assert torch.equal(state.buf, words)           # attention reads the state, only the sampler advances it
    # row b is bit-identical to a call in which every row is at p_b
    for b, p in enumerate(positions):
        cache.data.copy_(before)
        yu = D.decode_attention(qkv, cache, 0, D.DecodeState(dev, pos=p))
        assert torch.equal(y[b], yu[b]), (positions, b)
    cache.data.copy_(before)
    assert torch.equal(D.decode_attention(qkv, cache, 0, state), y)      # a second run: the same bits
    assert torch.equal(cache.data, expect)


def test_decode_embed_per_row_positions():
    g = torch.Generator().manual_seed(4)
    Vp, C, n_pos, B = 1024, 128, 512, 5
    wte = torch.randn(Vp, C, generator=g).to(dev, BF16)
    wpe = torch.randn(n_pos, C, generator=g).to(dev, BF16)
    tok = torch.randint(0, 1000, (B,), generator=g).to(dev)
    positions = (300, 0, 511, 128, 7)
    x = D.decode_embed(tok, wte, wpe, _state(positions))
    for b, p in enumerate(positions):
        xu = D.decode_embed(tok, wte, wpe, D.DecodeState(dev, pos=p))
        assert torch.equal(x[b], xu[b]), b
        assert rel_err(x[b], wte[tok[b]].float() + wpe[p].float()) < 1e-2, b


def test_sampler_bookkeeping_with_row_offsets():
    B, V, Vp, T0, n_new = 5, 1000, 1024, 4, 3
    offs = (0, -3, -1, 0, -2)
    g = torch.Generator().manual_seed(5)
    lgs = [(torch.randn(B, Vp, generator=g) * 3).to(BF16) for _ in range(2)]
    rng = DeviceRNG(31)
    for _ in range(6):
        rng.next()                                       # a draw number other than 0
    state = D.DecodeState(dev, rng.state.to(dev), pos=9, step=0, row_offsets=offs)
    nxt = torch.zeros(B, device=dev, dtype=torch.int64)
    out = torch.full((B, T0 + n_new), -1, device=dev, dtype=torch.int64)
    lout = torch.zeros(B, n_new, V, device=dev, dtype=BF16)
    ref0 = sample_reference(lgs[0], V, rng.next(), 0.9, 40, top_p=0.9)
    ref1 = sample_reference(lgs[1], V, rng.next(), 0.9, 40, top_p=0.9)
    eos = int(ref0[0])                                   # row 0 finishes at the first call
    assert eos not in ref0[1:].tolist() and eos not in ref1[1:].tolist()
    for lg in lgs:
        D.sample(lg.to(dev), V, state, 0.9, 40, eos, next=nxt, out=out, logits_out=lout, T0=T0, top_p=0.9)
    ref1[0] = eos
    expect = torch.full((B, T0 + n_new), -1, dtype=torch.int64)
    for b, off in enumerate(offs):
        expect[b, T0 + off], expect[b, T0 + off + 1] = ref0[b], ref1[b]
    assert torch.equal(out.cpu(), expect)                # the tokens at T0 + off_b + step, every other slot untouched
    assert torch.equal(nxt.cpu(), ref1)
    assert state.finished.cpu().tolist() == [1] + [0] * 15
    assert state.row_offsets.cpu().tolist() == list(offs) + [0] * 11
    assert torch.equal(lout.cpu()[:, 0], lgs[0][:, :V]) and torch.equal(lout.cpu()[:, 1], lgs[1][:, :V])
    assert (lout.cpu()[:, 2] == 0).all()                 # the logits slot is the step, not the position
    assert state.pos() == 11 and state.step() == 2 and state.row_pos(B) == [11 + o for o in offs]
    assert torch.equal(state.rng.cpu(), rng.state)       # the same seed and stream, draw number + 2


# --------------------------------------------------------------------------------------- sampler: top-p
@functools.lru_cache(maxsize=None)
def _reference(B, V, Vp):
    """Per setting: (snapshot, tokens, info) of the reference, computed once."""
    lg = GC.sampler_logits(B, V, Vp)
    res = []
    for i, (t, k, p) in enumerate(GC.TOPP_SETTINGS):
        snap = GC.topp_snapshot(B, V, i)
        res.append((snap,) + sample_reference(lg, V, snap, t, k, top_p=p, return_info=True))
    return lg, res


@functools.lru_cache(maxsize=None)
def _close_cases():
    return sum(int((info["p_slack"] < GC.P_SLACK).sum()) for s in GC.SAMPLER_SHAPES for _, _, info in _reference(*s)[1])


@pytest.mark.parametrize("B,V,Vp", GC.SAMPLER_SHAPES)
def test_sampler_top_p_matches_reference(B, V, Vp):
    """The device threshold equals the reference's exactly wherever the target mass ``top_p * W`` is at
    least 1e-4 of ``W`` away from a boundary between two thresholds; closer than that (at most 16 of the 528
    cases) it lies in the bracket of ``top_p +- 1e-4``.  1e-4: the fp32 error of a weight is dominated by the
    rounding of ``z`` and ``z - z_max``, about 2e-6 for ``|z| <= 20``; ``expf`` adds about 2.4e-7 and the
    fixed point 2.3e-8; 1e-4 is more than ten times their sum, the factor of the existing gap rule.  The
    token is then compared for the threshold the device chose."""
    assert _close_cases() <= GC.MAX_CLOSE_CASES, "a broken kernel must not be able to hide in the bracket class"
    lg, refs = _reference(B, V, Vp)
    lgd = lg.to(dev)
    for (t, k, p), (snap, _, info) in zip(GC.TOPP_SETTINGS, refs):
        thr = torch.full((B,), -1, device=dev, dtype=torch.int32)
        tok = D.sample(lgd, V, snap.to(dev), t, k, threshold_out=thr, top_p=p).cpu()
        got = D.key16_to_float(thr)
        exact = info["p_slack"] >= GC.P_SLACK
        lo, hi = info["threshold_p_bracket"]
        print(f"B {B} V {V} T {t} k {k} p {p}: exact class {int(exact.sum())}/{B}, "
              f"equal {int((got == info['threshold']).sum())}/{B}, min slack {info['p_slack'].min():.2e}")
        assert (got[exact] == info["threshold"][exact]).all(), (t, k, p, got, info["threshold"])
        assert ((lo <= got) & (got <= hi))[~exact].all(), (t, k, p, got, lo, hi)
        ref, rinfo = sample_reference(lg, V, snap, t, k, _threshold=got, return_info=True)
        close = rinfo["gap"] < GC.GAP
        assert not close.any(), (t, k, p, rinfo["gap"].min())
        differ = (tok != ref).numpy()
        assert not (differ & ~close).any() and differ.sum() <= 1, (t, k, p, tok, ref)
        if B >= 3:
            assert got[1] == 0.75 and rinfo["ncand"][1] == V       # the all-equal row keeps all V
        thr2 = torch.full((B,), -1, device=dev, dtype=torch.int32)
        tok2 = D.sample(lgd, V, snap.to(dev), t, k, threshold_out=thr2, top_p=p).cpu()
        assert torch.equal(tok, tok2) and torch.equal(thr, thr2)   # two calls: equal bits


@pytest.mark.parametrize("B,V,Vp", [(5, 1000, 1024), (16, 50257, 50304)])
def test_sampler_top_p_off_and_greedy(B, V, Vp):
    lgd = GC.sampler_logits(B, V, Vp).to(dev)
    snap = GC.topp_snapshot(B, V, 0).to(dev)
    for k in (None, 50):
        res = []
        for p in (None, 1.0):
            thr = torch.full((B,), -1, device=dev, dtype=torch.int32)
            res.append((D.sample(lgd, V, snap, 0.7, k, threshold_out=thr, top_p=p), thr))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert torch.equal(D.sample(lgd, V, snap, 0.0, k, top_p=0.5), D.sample(lgd, V, snap, 0.0, k))
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError):
            D.sample(lgd, V, snap, 1.0, top_p=bad)


# --------------------------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def twins():
    """bf16 GPU model and an fp32 CPU twin with identical (bf16-representable) weights."""
    g = build_gpt2(GC.tiny_cfg(), seed=0, device=dev)
    c = build_gpt2(GC.tiny_cfg(), seed=0, dtype=torch.float32)
    with torch.no_grad():
        for pc, pg in zip(c.parameters(), g.parameters()):
            pc.copy_(pg.float())
    return g, c


def _teacher_forced_failures(g, c, lens, n_new, after_prefill=None, pad=3):
    """``test_generate_gpu._teacher_forced_failures`` row by row: the twin sees row ``b``'s own tokens,
    unpadded, and its logits rows ``len_b - 1 + s`` are compared with the step-``s`` logits of the GPU."""
    idx = GC.ragged_prompt(lens, width=max(lens) + 2)
    W = idx.shape[1]
    out, lg = g.generate(idx.to(dev), n_new, temperature=0.0, return_logits=True, prompt_lens=list(lens),
                         pad_token_id=pad, _after_prefill=after_prefill)
    out, lg = out.cpu(), lg.float().cpu()
    assert out.shape == (len(lens), W + n_new) and lg.shape == (len(lens), n_new, 1000)
    fails = []
    for b, n in enumerate(lens):
        assert torch.equal(out[b, :n], idx[b, :n]) and (out[b, n + n_new:] == pad).all()
        assert torch.equal(out[b, n:n + n_new], lg[b].argmax(-1)), "token != lowest-index argmax of the returned logits"
        with torch.no_grad():
            ref = c(out[b:b + 1, :n + n_new - 1])[0]
        for s in range(n_new):
            x, y = lg[b, s].double(), ref[n - 1 + s].double()
            cs = F.cosine_similarity(x, y, dim=0).item()
            e = ((x - y).norm() / y.norm()).item()
            if not (cs >= 0.995 and e < 3e-2):
                fails.append((b, f"row {b} step {s}: cos {cs:.5f}, rel L2 err {e:.3e}"))
    return fails


@pytest.mark.parametrize("lens,n_new", [((5, 1, 9), 4), ((127, 128, 3), 3), ((130, 2, 64), 3), ((120, 7, 128), 140)])
def test_ragged_generate_matches_teacher_forced_twin(twins, lens, n_new):
    fails = _teacher_forced_failures(*twins, lens, n_new)
    assert not fails, fails


def test_ragged_check_catches_a_zeroed_cache_row_of_the_shortest_row(twins):
    lens = (5, 1, 9)
    short = lens.index(min(lens))

    def zero_row(cache):
        cache.data[:, :, short, :, lens[short] - 1] = 0

    fails = _teacher_forced_failures(*twins, lens, 4, after_prefill=zero_row)
    assert any(b == short for b, _ in fails), "a zeroed KV cache row of the shortest prompt went unnoticed"
    assert all(b == short for b, _ in fails), fails          # the other rows never read it


def test_ragged_graph_replay_equals_eager(twins):
    g, _ = twins
    lens = [7, 2, 12]
    idx = GC.ragged_prompt(lens).to(dev)
    a, la = g.generate(idx, 12, temperature=0.0, return_logits=True, prompt_lens=lens)
    b, lb = g.generate(idx, 12, temperature=0.0, return_logits=True, prompt_lens=lens, use_graph=False)
    assert torch.equal(a, b) and torch.equal(la, lb)
    kw = dict(temperature=0.8, top_k=40, top_p=0.9, seed=11, prompt_lens=lens, return_logits=True)
    a, la = g.generate(idx, 12, **kw)
    b, lb = g.generate(idx, 12, use_graph=False, **kw)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_uniform_prompt_lens_equal_the_call_without_them(twins):
    g, _ = twins
    idx = GC.ragged_prompt((7, 7, 7)).to(dev)
    for kw in (dict(temperature=0.8, top_k=40, seed=11), dict(temperature=0.8, top_k=40, top_p=0.9, seed=11),
               dict(temperature=0.0)):
        a, la = g.generate(idx, 12, return_logits=True, **kw)
        b, lb = g.generate(idx, 12, return_logits=True, prompt_lens=[7, 7, 7], **kw)
        assert torch.equal(a, b) and torch.equal(la, lb), kw
    a = g.generate(idx, 12, temperature=0.8, seed=11)
    assert torch.equal(a, g.generate(idx, 12, temperature=0.8, seed=11, top_p=1.0))


def test_ragged_limits_and_side_effects(twins):
    g, _ = twins
    lens = [5, 1, 9]
    idx = GC.ragged_prompt(lens).to(dev)
    params = [p.detach().clone() for p in g.parameters()]
    g.seed_dropout(4)
    draw = g.rng.draw_number()
    g.train()
    gen = DeviceRNG(13, device=dev)
    g.generate(idx, 6, temperature=1.0, top_p=0.9, prompt_lens=lens, generator=gen)
    assert g.training and gen.draw_number() == 6         # one draw number per token, whatever the lengths
    for bad in ([5, 0, 9], [5, 1, 10], [5, 1], [5, 1, 9, 2]):
        with pytest.raises(ValueError):
            g.generate(idx, 2, prompt_lens=bad)
    wide = GC.ragged_prompt((5, 1, 500), width=510).to(dev)
    with pytest.raises(ValueError):
        g.generate(wide, 13, prompt_lens=[5, 1, 500])    # 500 + 13 > block_size
    for pad in (-1, 1000):
        with pytest.raises(ValueError):
            g.generate(idx, 2, prompt_lens=lens, pad_token_id=pad)
    for p in (0.0, 1.01):
        with pytest.raises(ValueError):
            g.generate(idx, 2, top_p=p)
    with pytest.raises(NotImplementedError):
        g.generate(GC.ragged_prompt([3] * 17).to(dev), 2, prompt_lens=[3] * 17)
    assert g.training
    g.eval()
    assert g.rng.draw_number() == draw
    assert all(torch.equal(p, q) for p, q in zip(g.parameters(), params))
