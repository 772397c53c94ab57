"""Dropout fused into the HIP kernels (embedding, add + LayerNorm, flash attention) against fp32
references that use the SAME mask (drawn on the CPU from ops/rng.py), whole-model parity under
dropout, and mask renewal across hipGraph replays."""
import math

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import DeviceRNG, effective_p, rng as R
from pytorch_distributed_example_amd.ops import transformer as T
from pytorch_distributed_example_amd.optim import AdamWMaster

pytestmark = pytest.mark.gpu
dev = "cuda"


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _snaps(seed=77, draw=0, stream=0):
    """The same snapshot on the GPU (through the rng_next kernel) and on the CPU."""
    out = []
    for d in (dev, "cpu"):
        r = DeviceRNG(seed, stream, device=d)
        r.load_state_dict({"seed": seed, "draw": draw, "stream": stream})
        out.append(r.next())
    assert R.snapshot_words(out[0]) == R.snapshot_words(out[1])
    return out


# ------------------------------------------------------------------------------------ mask kernel
@pytest.mark.parametrize("shape", [(4 * 7,), (128, 768), (3, 5, 7)])
def test_mask_kernel_elementwise(shape):
    sg, sc = _snaps(seed=(5 << 32) + 9, draw=3, stream=2)
    for p in (0.1, 0.5):
        got = R.dropout_mask(sg, 4, p, shape=shape)
        assert got.is_cuda and got.dtype == torch.uint8
        assert torch.equal(got.cpu(), R.dropout_mask(sc, 4, p, shape=shape))


@pytest.mark.parametrize("B,H,Tn", [(1, 1, 128), (2, 3, 256)])
def test_mask_kernel_attention(B, H, Tn):
    sg, sc = _snaps(seed=123456789012345, draw=1, stream=1)
    got = R.dropout_mask(sg, 7, 0.1, bht=(B, H, Tn))
    want = R.dropout_mask(sc, 7, 0.1, bht=(B, H, Tn))
    assert torch.equal(got.cpu(), want)
    assert abs(want.float().mean().item() - (1 - 25 / 256)) < 5 * math.sqrt(0.1 * 0.9 / want.numel())


def test_device_rng_next_on_gpu():
    r = DeviceRNG(seed=(3 << 32) | 4, stream=6, device=dev)
    s0, s1 = r.next(), r.next()
    assert R.snapshot_words(s0) == (4, 3, 0, 6) and R.snapshot_words(s1) == (4, 3, 1, 6)
    assert r.state_dict() == {"seed": (3 << 32) | 4, "draw": 2, "stream": 6}


# ------------------------------------------------------------------------------------ embedding
def test_embedding_dropout():
    torch.manual_seed(3)
    B, Tn, C, Vp, p = 2, 128, 128, 512, 0.1                   # N = B * T = 256 rows
    sg, sc = _snaps()
    idx = torch.randint(0, 40, (B, Tn), device=dev)
    wte = torch.randn(Vp, C).to(dev, torch.bfloat16).requires_grad_()
    wpe = torch.randn(Tn, C).to(dev, torch.bfloat16).requires_grad_()
    x = T.embedding(idx, wte, wpe, p, sg, 0)
    g = torch.randn(B, Tn, C).to(dev, torch.bfloat16)
    x.backward(g)
    mask = R.dropout_mask(sc, 0, p, shape=(B, Tn, C)).to(dev).bool()
    assert 0 < (~mask).sum().item() < mask.numel()
    wter, wper = wte.detach().float().requires_grad_(), wpe.detach().float().requires_grad_()
    xr = (F.embedding(idx, wter) + wper.unsqueeze(0)) * mask.float() / (1 - effective_p(p))
    xr.backward(g.float())
    assert (x[~mask] == 0).all()
    assert rel_err(x[mask], xr[mask]) < 1e-2
    assert rel_err(wte.grad, wter.grad) < 2e-2
    assert rel_err(wpe.grad, wper.grad) < 2e-2


# ------------------------------------------------------------------------------------ residual site
@pytest.mark.parametrize("N,C", [(7, 2048), (96, 384), (300, 768)])
def test_add_dropout_layer_norm_residual(N, C):
    torch.manual_seed(11)
    p, site = 0.1, 5
    sg, sc = _snaps(draw=2)
    mk = lambda *s: torch.randn(*s).to(dev, torch.bfloat16).requires_grad_()
    x, d = mk(N, C), mk(N, C)
    w = (1 + 0.1 * torch.randn(C)).to(dev, torch.bfloat16).requires_grad_()
    b = (0.1 * torch.randn(C)).to(dev, torch.bfloat16).requires_grad_()
    s, y = T.add_dropout_layer_norm_residual(x, d, w, b, 1e-5, p, sg, site)
    gs, gy = (torch.randn(N, C).to(dev, torch.bfloat16) for _ in range(2))
    torch.autograd.backward([s, y], [gs, gy])
    mask = R.dropout_mask(sc, site, p, shape=(N, C)).to(dev).bool()
    assert 0 < (~mask).sum().item() < mask.numel()
    xr, dr, wr, br = (t.detach().float().requires_grad_() for t in (x, d, w, b))
    sr = xr + dr * mask.float() / (1 - effective_p(p))
    yr = F.layer_norm(sr, (C,), wr, br, 1e-5)
    torch.autograd.backward([sr, yr], [gs.float(), gy.float()])
    assert torch.equal(s[~mask], x.detach()[~mask])            # dropped: s == x exactly
    assert rel_err(s, sr) < 1e-2
    assert rel_err(y, yr) < 1e-2
    assert (d.grad[~mask] == 0).all()                          # dD exactly 0 where dropped
    assert rel_err(x.grad, xr.grad) < 2e-2
    assert rel_err(d.grad, dr.grad) < 2e-2
    assert rel_err(w.grad, wr.grad) < 2e-2
    assert rel_err(b.grad, br.grad) < 2e-2


# ------------------------------------------------------------------------------------ attention
def _attn_ref(qkv, H, mask=None, keep=1.0):
    B, Tn, C3 = qkv.shape
    C = C3 // 3
    q, k, v = qkv.float().split(C, dim=2)
    q, k, v = (t.reshape(B, Tn, H, C // H).transpose(1, 2) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(C // H)
    causal = torch.triu(torch.ones(Tn, Tn, dtype=torch.bool, device=qkv.device), 1)
    pr = torch.softmax(s.masked_fill(causal, float("-inf")), -1)
    if mask is not None:
        pr = pr * mask.float() / keep                          # materialised mask, after the softmax
    return (pr @ v).transpose(1, 2).reshape(B, Tn, C)


def _check_attention_dropout(B, Tn, H):
    torch.manual_seed(4)
    p, site, C = 0.1, 4, 64 * H
    sg, sc = _snaps(draw=5, stream=1)
    qkv = torch.randn(B, Tn, 3 * C).to(dev, torch.bfloat16).requires_grad_()
    y = T.causal_attention(qkv, H, p, sg, site)
    g = torch.randn(B, Tn, C).to(dev, torch.bfloat16)
    y.backward(g)
    mask = R.dropout_mask(sc, site, p, bht=(B, H, Tn)).to(dev)
    qr = qkv.detach().float().requires_grad_()
    yr = _attn_ref(qr, H, mask, 1 - effective_p(p, "attention"))
    yr.backward(g.float())
    dq, dk, dv = qkv.grad.split(C, dim=2)
    rq, rk, rv = qr.grad.split(C, dim=2)
    errs = dict(y=rel_err(y, yr), dv=rel_err(dv, rv), dk=rel_err(dk, rk), dq=rel_err(dq, rq))
    print("attention dropout errors", (B, Tn, H), errs)
    assert errs["y"] < 2e-2
    assert errs["dv"] < 3e-2
    assert errs["dk"] < 3e-2
    assert errs["dq"] < 3e-2
    # and the output really is dropped (differs from the p = 0 reference by far more than the bound)
    assert rel_err(y, _attn_ref(qkv.detach(), H)) > 5e-2


@pytest.mark.parametrize("B,Tn,H", [(1, 128, 1), (2, 256, 3), (3, 384, 7)])
def test_flash_attention_dropout(B, Tn, H):
    _check_attention_dropout(B, Tn, H)


def test_flash_attention_dropout_deep_ring_forward():
    """attn_set_variant(0): the 4-deep-ring, 2-blocks-per-CU forward has its own DROP instantiation."""
    from pytorch_distributed_example_amd._ext import kernels
    try:
        kernels().attn_set_variant(0)
        _check_attention_dropout(2, 256, 3)
    finally:
        kernels().attn_set_variant(5)


def test_flash_attention_dropout_block_maps_agree():
    from pytorch_distributed_example_amd._ext import kernels
    K = kernels()
    torch.manual_seed(6)
    B, Tn, H = 3, 384, 7
    C = 64 * H
    sg, _ = _snaps(draw=1)
    qkv = torch.randn(B, Tn, 3 * C).to(dev, torch.bfloat16)
    g = torch.randn(B, Tn, C).to(dev, torch.bfloat16)
    outs = []
    try:
        for grp in (255, 0, 3, 16):
            K.attn_set_variant(5 | (grp << 8))
            x = qkv.clone().requires_grad_()
            y = T.causal_attention(x, H, 0.1, sg, 2)
            y.backward(g)
            outs.append((y.detach(), x.grad))
    finally:
        K.attn_set_variant(5)
    for y, dx in outs[1:]:
        assert torch.equal(y, outs[0][0]) and torch.equal(dx, outs[0][1])


def test_flash_attention_p0_is_the_existing_path():
    torch.manual_seed(7)
    B, Tn, H = 2, 256, 3
    sg, _ = _snaps()
    qkv = torch.randn(B, Tn, 3 * 64 * H).to(dev, torch.bfloat16)
    g = torch.randn(B, Tn, 64 * H).to(dev, torch.bfloat16)
    a = qkv.clone().requires_grad_()
    b = qkv.clone().requires_grad_()
    ya = T.causal_attention(a, H)
    yb = T.causal_attention(b, H, p=0.0, rng_snapshot=sg, site=3)
    ya.backward(g)
    yb.backward(g)
    assert torch.equal(ya, yb) and torch.equal(a.grad, b.grad)


# ------------------------------------------------------------------------------------ whole model
def _gpt2_dropout_parity(twin_seed: int):
    """tests/test_transformer_gpu.py::_gpt2_parity (4 layers, d 128, T 128, B 4; same thresholds) with
    all three probabilities at 0.1: the GPU bf16 model is seeded 21, its fp32 CPU twin `twin_seed`."""
    pd = 0.1
    cfg = GPTConfig(block_size=128, vocab_size=1000, padded_vocab=1024, n_layer=4, n_head=2, n_embd=128,
                    embd_pdrop=pd, attn_pdrop=pd, resid_pdrop=pd)
    g = build_gpt2(cfg, seed=0, device=dev).seed_dropout(21)
    c = build_gpt2(cfg, seed=0, dtype=torch.float32).seed_dropout(twin_seed)
    with torch.no_grad():
        for pc, pg in zip(c.parameters(), g.parameters()):
            pc.copy_(pg.float())
    torch.manual_seed(5)
    idx = torch.randint(0, cfg.vocab_size, (4, 128))
    tgt = torch.randint(0, cfg.vocab_size, (4, 128))

    def streams(m, i):
        t = m.transformer
        snap = m.rng.next()
        x = T.embedding(i, t.wte.weight, t.wpe.weight, pd, snap, 0)
        delta, out = None, []
        for l, blk in enumerate(t.h):
            x, delta = blk.forward_deferred(x, delta, snap)
            keep = R.dropout_mask(snap, 3 + 3 * l, pd, shape=delta.shape).float() / (1 - effective_p(pd))
            out.append((x.float() + delta.float() * keep).detach())
        return out

    with torch.no_grad():
        sg, sc = streams(g, idx.to(dev)), streams(c, idx)
    fails = []
    for k, (a, b) in enumerate(zip(sg, sc)):
        cs = F.cosine_similarity(a.double().flatten().cpu(), b.double().flatten(), dim=0).item()
        e = ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()
        if not (cs >= 0.995 and e < 3e-2):
            fails.append(f"block {k} residual stream: cos {cs:.5f}, rel L2 err {e:.3e}")
    lg = g(idx.to(dev), tgt.to(dev))
    lc = c(idx, tgt)
    lg.backward()
    lc.backward()
    if not abs(lg.item() - lc.item()) < 1e-2:
        fails.append(f"loss {lg.item():.5f} vs {lc.item():.5f}")
    for (n, pg), pc in zip(g.named_parameters(), c.parameters()):
        cos = F.cosine_similarity(pg.grad.float().flatten().cpu(), pc.grad.flatten(), dim=0).item()
        if not cos >= 0.99:
            fails.append(f"grad {n}: cos {cos:.4f}")
    assert g.rng.draw_number() == 2 and c.rng.draw_number() == 2
    return fails


def test_gpt2_dropout_gpu_matches_cpu_fp32():
    fails = _gpt2_dropout_parity(twin_seed=21)
    assert not fails, fails


def test_gpt2_dropout_parity_catches_wrong_mask():
    fails = _gpt2_dropout_parity(twin_seed=22)
    assert fails, "a twin that drops other elements went unnoticed"


def test_gpt2_dropout_off_draws_nothing():
    cfg = GPTConfig(block_size=128, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128,
                    resid_pdrop=0.1)
    m = build_gpt2(cfg, seed=1, device=dev).seed_dropout(3)
    ref = build_gpt2(GPTConfig(block_size=128, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128),
                     seed=1, device=dev)
    idx = torch.randint(0, 1000, (2, 128), device=dev)
    m.eval()
    assert torch.equal(m(idx, idx), ref(idx, idx)) and m._rng is None
    m.train()
    assert not torch.equal(m(idx, idx), ref(idx, idx)) and m.rng.draw_number() == 1


# ------------------------------------------------------------------------------------ hipGraph
def test_gpt2_dropout_step_replays_with_fresh_masks():
    """One captured step (capturable AdamW, dropout 0.1), replayed three times on ONE batch: every
    replay draws a new mask on the device, and the run equals the same steps done eagerly."""
    cfg = GPTConfig(block_size=128, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128,
                    embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1)
    torch.manual_seed(9)
    batches = [torch.randint(0, cfg.vocab_size, (2, 129), device=dev) for _ in range(3)]

    def run(graph_mode):
        m = build_gpt2(cfg, seed=2, device=dev).seed_dropout(31)
        opt = AdamWMaster(m.decay_groups(0.1), lr=3e-3, max_grad_norm=1.0, capturable=graph_mode)

        def one(b):
            opt.zero_grad()
            loss = m(b[:, :-1], b[:, 1:])
            loss.backward()
            opt.step()
            return loss.detach()

        losses = [one(batches[0]).item(), one(batches[1]).item()]      # two eager steps first
        if not graph_mode:
            losses += [one(batches[2]).item() for _ in range(3)]
        else:
            sb = batches[2].clone()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                sl = one(sb)
            for _ in range(3):
                g.replay()
                losses.append(sl.item())
        torch.cuda.synchronize()
        return losses, [p.detach().float().clone() for p in m.parameters()], m

    le, pe, _ = run(False)
    lg, pg, m = run(True)
    r = lg[2:]
    assert r[0] != r[1] and r[1] != r[2] and r[0] != r[2], r      # a new mask on every replay
    assert le == pytest.approx(lg, rel=2e-3)
    for a, b in zip(pe, pg):
        assert rel_err(a, b) < 1e-2
    assert m.rng.draw_number() == 5
