"""Dropout RNG on the CPU: Philox known answers, mask statistics, DeviceRNG bookkeeping and the GPT-2
plumbing (the CPU ops draw their masks from the same definition the HIP kernels use)."""
import math

import numpy as np
import pytest
import torch

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import DeviceRNG, effective_p, rng as R
from pytorch_distributed_example_amd.ops import transformer as T

N = 1 << 20


def _snap(seed=1234, draw=0, stream=0):
    r = DeviceRNG(seed, stream)
    r.load_state_dict({"seed": seed, "draw": draw, "stream": stream})
    return r.next()


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expect):
    out = R.philox4x32_10(counter, key)
    assert " ".join(f"{int(w):08x}" for w in out) == expect
    # the vectorised form gives the same words at every position of an array
    arr = R.philox4x32_10([np.full(5, c, dtype=np.uint64) for c in counter], key)
    assert all((a == o).all() for a, o in zip(arr, out))


def test_addressing_matches_header_table():
    """key = seed, counter = (group lo, group hi, draw, site | stream << 16): pde_rng.h."""
    seed, draw, stream, site = 0x0123456789ABCDEF, 7, 3, 11
    s = _snap(seed, draw, stream)
    assert R.snapshot_words(s) == (0x89ABCDEF, 0x01234567, 7, 3)
    g = (1 << 32) + 5          # exercises counter word 1
    want = R.philox4x32_10((g & 0xFFFFFFFF, g >> 32, draw, site | (stream << 16)), (0x89ABCDEF, 0x01234567))
    got = R._words(s, site, np.array([g], dtype=np.uint64))
    assert [int(w[0]) for w in got] == [int(w) for w in want]
    thr = R.threshold(0.3)
    m = R.elementwise_mask(s, site, 8, 0.3)
    w0 = R.philox4x32_10((0, 0, draw, site | (stream << 16)), (0x89ABCDEF, 0x01234567))
    assert m[:4].tolist() == [int(int(w) >= thr) for w in w0]
    # attention: byte (k & 3) of word (q & 3) of group (bh * T/4 + q/4) * T/4 + k/4
    Tn = 8
    am = R.attention_mask(s, site, 1, 2, Tn, 0.3)
    bh, q, k = 1, 6, 5
    grp = (bh * 2 + q // 4) * 2 + k // 4
    w = R.philox4x32_10((grp, 0, draw, site | (stream << 16)), (0x89ABCDEF, 0x01234567))
    byte = (int(w[q & 3]) >> (8 * (k & 3))) & 0xFF
    assert int(am[0, 1, q, k]) == int(byte >= R.threshold(0.3, "attention"))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    kept = R.elementwise_mask(_snap(), 0, N, p).sum().item()
    assert abs(kept / N - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / N)
    # attention sites realise effective_p (8-bit threshold), which is what their 1 / keep uses
    pe = effective_p(p, "attention")
    assert pe == math.floor(p * 256) / 256
    ka = R.attention_mask(_snap(), 0, 4, 4, 256, p)
    assert abs(ka.float().mean().item() - (1 - pe)) <= 5 * math.sqrt(pe * (1 - pe) / ka.numel())


def test_effective_p():
    assert effective_p(0.1, "elementwise") == math.floor(0.1 * 2 ** 32) / 2 ** 32
    assert effective_p(0.1, "attention") == 25 / 256
    assert effective_p(0.5, "attention") == 0.5 and effective_p(0.0, "attention") == 0.0
    assert R.inv_keep(0.1, "attention") == 1 / (1 - 25 / 256)
    with pytest.raises(ValueError):
        effective_p(1.0)
    with pytest.raises(ValueError):
        effective_p(0.1, "rows")


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("vary", ["site", "draw", "stream"])
def test_independence(vary, p):
    base = dict(seed=99, draw=4, stream=2)
    other = dict(base)
    site_a = site_b = 5
    if vary == "site":
        site_b = 6
    else:
        other[vary] += 1
    a = R.elementwise_mask(_snap(**base), site_a, N, p)
    b = R.elementwise_mask(_snap(**other), site_b, N, p)
    agree = (a == b).float().mean().item()
    exp = p * p + (1 - p) * (1 - p)
    assert abs(agree - exp) <= 5 * math.sqrt(exp * (1 - exp) / N)
    assert torch.equal(a, R.elementwise_mask(_snap(**base), site_a, N, p))     # same snapshot and site: same mask


def test_independence_attention_sites():
    p = 0.5
    a = R.attention_mask(_snap(5, 1, 0), 1, 2, 4, 256, p)
    n = a.numel()
    for snap, site in ((_snap(5, 1, 0), 4), (_snap(5, 2, 0), 1), (_snap(5, 1, 1), 1)):
        agree = (a == R.attention_mask(snap, site, 2, 4, 256, p)).float().mean().item()
        assert abs(agree - 0.5) <= 5 * math.sqrt(0.25 / n)
    assert torch.equal(a, R.attention_mask(_snap(5, 1, 0), 1, 2, 4, 256, p))


def test_device_rng_state():
    r = DeviceRNG(seed=(1 << 40) + 17, stream=3)
    s0 = r.next()
    s1 = r.next()
    assert R.snapshot_words(s0) == (17, 1 << 8, 0, 3)
    assert R.snapshot_words(s1)[2] == 1 and r.draw_number() == 2
    assert R.snapshot_words(s0)[2] == 0                      # a later draw leaves earlier snapshots alone
    sd = r.state_dict()
    assert sd == {"seed": (1 << 40) + 17, "draw": 2, "stream": 3}
    r2 = DeviceRNG()
    r2.load_state_dict(sd)
    assert torch.equal(r2.next(), r.next())
    r.manual_seed(5)
    assert r.state_dict() == {"seed": 5, "draw": 0, "stream": 3}
    with pytest.raises(ValueError):
        DeviceRNG(0, stream=1 << 16)


# ------------------------------------------------------------------------------------ tiny GPT
def _tiny_cfg(**kw):
    return GPTConfig(block_size=128, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128, **kw)


_P = dict(embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1)


@pytest.fixture(scope="module")
def batch():
    torch.manual_seed(8)
    idx = torch.randint(0, 1000, (2, 128))
    return idx, torch.roll(idx, -1, 1)


def _model(**kw):
    return build_gpt2(_tiny_cfg(**kw), seed=1, dtype=torch.float32)


def test_config_defaults_off():
    c = GPTConfig()
    assert (c.embd_pdrop, c.attn_pdrop, c.resid_pdrop) == (0.0, 0.0, 0.0)


def test_gpt_p0_is_bit_identical_and_draws_nothing(batch):
    a = _model()
    b = _model(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    la, lb = a(*batch), b(*batch)
    assert torch.equal(la, lb)
    la.backward()
    lb.backward()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa.grad, pb.grad)
    assert b._rng is None                                     # no RNG, no next(), no snapshot
    assert not any("rng" in k for k in b.state_dict())        # and never a module buffer
    assert not list(b.buffers())


def test_gpt_dropout_train_eval_and_reproducibility(batch):
    base = _model()(*batch)
    m = _model(**_P).seed_dropout(7)
    l1 = m(*batch)
    l2 = m(*batch)
    assert l1.item() != base.item() and l2.item() != l1.item()   # dropped, and a new mask per forward
    assert m.rng.draw_number() == 2
    m.eval()
    assert torch.equal(m(*batch), base)                          # eval: the p = 0 loss exactly
    assert m.rng.draw_number() == 2                              # ... and no draw
    m.train()
    m.seed_dropout(7)
    assert torch.equal(m(*batch), l1) and torch.equal(m(*batch), l2)    # one seed reproduces
    n = _model(**_P).seed_dropout(7, stream=1)
    assert n(*batch).item() != l1.item()                         # another stream: other masks


def test_gpt_rng_state_dict_continues_sequence(batch):
    m = _model(**_P).seed_dropout(3)
    m(*batch)
    sd = m.rng.state_dict()
    assert sd == {"seed": 3, "draw": 1, "stream": 0}
    want = [m(*batch), m(*batch)]
    n = _model(**_P)
    n.rng.load_state_dict(sd)
    assert torch.equal(n(*batch), want[0]) and torch.equal(n(*batch), want[1])


def test_second_forward_keeps_first_masks(batch):
    m = _model(**_P).seed_dropout(11)
    la = m(*batch)
    m(*batch)                       # a second forward before the first backward
    la.backward()
    ga = [p.grad.clone() for p in m.parameters()]
    n = _model(**_P).seed_dropout(11)
    n(*batch).backward()
    for a, p in zip(ga, n.parameters()):
        assert torch.equal(a, p.grad)


def test_residual_dropout_gradients():
    torch.manual_seed(0)
    Nr, C, p, site = 24, 64, 0.25, 9
    snap = _snap(42, 3, 1)
    x = torch.randn(Nr, C, requires_grad=True)
    d = torch.randn(Nr, C, requires_grad=True)
    w = torch.randn(C, requires_grad=True)
    b = torch.randn(C, requires_grad=True)
    s, y = T.add_dropout_layer_norm_residual(x, d, w, b, 1e-5, p, snap, site)
    (s * torch.randn(Nr, C) + y * torch.randn(Nr, C)).sum().backward()
    mask = R.dropout_mask(snap, site, p, shape=(Nr, C)).bool()
    assert 0 < (~mask).sum() < mask.numel()
    assert torch.equal(s.detach()[~mask], x.detach()[~mask])
    assert (d.grad[~mask] == 0).all()                                        # dropped: exactly zero
    assert torch.equal(d.grad[mask], (x.grad * R.inv_keep(p))[mask])         # kept: dX / keep
    # p = 0 is the undropped op
    s0, y0 = T.add_dropout_layer_norm_residual(x, d, w, b, 1e-5, 0.0, None, site)
    sr, yr = T.add_layer_norm_residual(x, d, w, b, 1e-5)
    assert torch.equal(s0, sr) and torch.equal(y0, yr)
    with pytest.raises(ValueError):
        T.add_dropout_layer_norm_residual(x, d, w, b, 1e-5, p, None, site)


def test_attention_and_embedding_cpu_definitions():
    torch.manual_seed(1)
    B, Tn, H, p = 2, 128, 2, 0.1
    snap = _snap(6, 0, 0)
    qkv = torch.randn(B, Tn, 3 * 64 * H)
    y0 = T.causal_attention(qkv, H)
    assert torch.equal(T.causal_attention(qkv, H, 0.0, None, 3), y0)
    y = T.causal_attention(qkv, H, p, snap, 3)
    # reference: materialised mask after the softmax, scaled by 1 / (1 - effective_p)
    q, k, v = (t.reshape(B, Tn, H, 64).transpose(1, 2) for t in qkv.split(64 * H, dim=2))
    s = (q @ k.transpose(-1, -2)) / 8.0
    s = s.masked_fill(torch.triu(torch.ones(Tn, Tn, dtype=torch.bool), 1), float("-inf"))
    m = R.dropout_mask(snap, 3, p, bht=(B, H, Tn)).float() / (1 - effective_p(p, "attention"))
    ref = ((torch.softmax(s, -1) * m) @ v).transpose(1, 2).reshape(B, Tn, 64 * H)
    assert torch.allclose(y, ref, atol=1e-6)
    assert not torch.allclose(y, y0, atol=1e-3)
    idx = torch.randint(0, 50, (B, Tn))
    wte, wpe = torch.randn(64, 32), torch.randn(Tn, 32)
    e0 = T.embedding(idx, wte, wpe)
    e = T.embedding(idx, wte, wpe, 0.5, snap, 0)
    me = R.dropout_mask(snap, 0, 0.5, shape=e0.shape).bool()
    assert (e[~me] == 0).all() and torch.equal(e[me], (e0 * R.inv_keep(0.5))[me])
