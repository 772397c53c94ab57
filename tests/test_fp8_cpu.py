"""FP8 forward, CPU side: the numeric definition (``ops.fp8.quantize_reference``), the CPU twin of ``linear_fp8`` and
a tiny GPT with ``fp8_forward=True``."""
import math

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import fp8


def _family(name, shape=(37, 48)):
    torch.manual_seed(1)
    t = torch.randn(shape)
    if name == "zero":
        t.zero_()
    elif name == "outlier":            # would be far above 448 without the scale; the rest flushes
        t.mul_(1e-3)
        t.view(-1)[5] = 3e4
    elif name == "pow2":               # amax an exact power of two
        t.clamp_(-3, 3)
        t.view(-1)[7] = -4.0
    elif name == "edge448":            # amax * s == 448 exactly
        t.clamp_(-1.5, 1.5)
        t.view(-1)[3] = 1.75
    elif name == "huge":               # s < 1, and t * s rounds up towards 448
        t.mul_(1e30)
    return t


@pytest.mark.parametrize("name", ["normal", "zero", "outlier", "pow2", "edge448", "huge"])
def test_quantize_reference(name):
    t = _family(name)
    q, scale = fp8.quantize_reference(t)
    s, inv = scale.tolist()
    assert q.dtype == torch.float8_e4m3fn and q.shape == t.shape
    assert math.frexp(s)[0] == 0.5 and s * inv == 1.0                 # a power of two and its exact inverse
    qf = q.float()
    assert torch.isfinite(qf).all()
    if name == "zero":
        assert s == 1.0 and (qf == 0).all()
        return
    assert 224 < qf.abs().max().item() <= 448
    if name == "edge448":
        assert qf.abs().max().item() == 448 and s == 256.0
    # within half an e4m3 ulp of t * s: 3 mantissa bits, smallest normal exponent -6
    ts = t.double() * s
    ulp = torch.exp2(torch.floor(torch.log2(ts.abs().clamp(min=2.0 ** -6))) - 3)
    assert ((qf.double() - ts).abs() <= ulp / 2).all()


def test_clamp_is_part_of_the_definition():
    """A value that is finite in bf16/fp32 but above 448 after scaling cannot occur by construction (amax * s <= 448);
    the clamp covers the cast's behaviour at the edge: torch's own cast of 500 is NaN, the definition's is 448."""
    assert torch.isnan(torch.tensor(500.0).to(torch.float8_e4m3fn).float())
    assert torch.tensor(500.0).clamp(-fp8.E4M3_MAX, fp8.E4M3_MAX).to(torch.float8_e4m3fn).float() == 448


@pytest.mark.parametrize("bias", [True, False])
def test_linear_fp8_cpu_twin(bias):
    torch.manual_seed(2)
    x = torch.randn(3, 5, 64, requires_grad=True)
    w = (0.1 * torch.randn(24, 64)).requires_grad_()
    b = torch.randn(24, requires_grad=True) if bias else None
    dy = torch.randn(3, 5, 24)
    y = fp8.linear_fp8(x, w, b)
    xq, wq = fp8.quantize_reference(x.reshape(-1, 64)), fp8.quantize_reference(w)
    want = F.linear(xq.data.float(), wq.data.float()) * (xq.scale[1] * wq.scale[1])
    want = want + b if bias else want
    assert torch.equal(y.detach(), want.detach().view(3, 5, 24))
    assert not torch.equal(y.detach(), F.linear(x, w, b).detach())       # it did quantise
    ins = [t for t in (x, w, b) if t is not None]
    got = torch.autograd.grad(y, ins, dy)
    ref = torch.autograd.grad(F.linear(x, w, b), ins, dy)               # straight-through
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def test_tiny_gpt_fp8_forward_cpu():
    cfg = GPTConfig(block_size=32, vocab_size=100, padded_vocab=128, n_layer=2, n_head=2, n_embd=64, fp8_forward=True)
    m = build_gpt2(cfg, seed=0, dtype=torch.float32)
    off = build_gpt2(GPTConfig(**{**cfg.__dict__, "fp8_forward": False}), seed=0, dtype=torch.float32)
    torch.manual_seed(3)
    idx, tgt = torch.randint(0, 100, (2, 32)), torch.randint(0, 100, (2, 32))
    loss = m(idx, tgt)
    loss.backward()
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    lo = off(idx, tgt)
    assert loss.item() != lo.item()                                            # the flag reached the projections
    # generate ignores the flag
    assert torch.equal(m.generate(idx[:, :4], 3, temperature=0.0), off.generate(idx[:, :4], 3, temperature=0.0))
