"""MXFP8 on the CPU: ``quantize_mx_reference`` against the definition written out per block, and the model's twin."""
import math

import pytest
import torch

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import fp8

FAMILIES = ["normal", "zero", "outlier", "pow2", "m1.75", "m1.875", "2^127", "2^-125"]


def _family(name, shape=(3, 96), seed=0):
    """As tests/test_mxfp8_gpu.py's: block g of row r times 2^((3 r + 5 g) % 11 - 5), then the family's edge."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g).unflatten(-1, (-1, 32))
    r, b = torch.arange(t.shape[0]).view(-1, 1), torch.arange(t.shape[1])
    ramp = (2.0 ** ((3 * r + 5 * b) % 11 - 5)).unsqueeze(-1)
    if name == "zero":
        t[:, 1::3, :] = 0.0
        t[:, 1::3, ::2] = -0.0
    elif name == "outlier":
        t.mul_(1e-3)
        t[:, 0, 7] = 3e4
    elif name == "pow2":
        t.clamp_(-3, 3)[..., 5] = -4.0
    elif name == "m1.75":
        t.clamp_(-1.5, 1.5)[..., 0] = -1.75
    elif name == "m1.875":
        t.clamp_(-1.5, 1.5)[..., 31] = 1.875
    elif name in ("2^127", "2^-125"):
        t.clamp_(-0.9, 0.9)[..., 3] = 1.0
        ramp = torch.tensor(2.0 ** 127 if name == "2^127" else 2.0 ** -125)
    return (t * ramp).flatten(-2).bfloat16()


@pytest.mark.parametrize("name", FAMILIES)
def test_reference_is_the_definition_per_block(name):
    t = _family(name)
    q = fp8.quantize_mx_reference(t)
    assert q.data.shape == t.shape and q.scale.shape == (3, 3) and q.scale.dtype == torch.uint8
    for r in range(3):
        for g in range(3):
            blk = t[r, 32 * g:32 * g + 32].float()
            amax, k = blk.abs().max().item(), 0
            if amax:
                m, e = math.frexp(amax)                 # m in [0.5, 1)
                k = min((8 if 2 * m <= 1.75 else 7) - (e - 1), 127)
            assert amax * 2.0 ** k <= 448 and (amax == 0 or k == 127 or amax * 2.0 ** (k + 1) > 448)
            want = (blk.double() * 2.0 ** k).clamp(-448, 448).float().to(fp8.E4M3)
            assert q.scale[r, g].item() == 127 - k and 0 <= 127 - k <= 247
            assert torch.equal(q.data[r, 32 * g:32 * g + 32].view(torch.uint8), want.view(torch.uint8))


@pytest.mark.parametrize("name", FAMILIES)
def test_dequantize_within_half_ulp_of_the_block_scale(name):
    """|dq - t| <= half an e4m3 ulp at |t| 2^k (2^-4 relative for normals, 2^-10 absolute below 2^-6), over 2^k."""
    t = _family(name).double()
    q = fp8.quantize_mx_reference(t)
    inv = torch.pow(2.0, q.scale.double() - 127.0).repeat_interleave(32, -1)
    scaled = (t / inv).abs()
    ulp = torch.where(scaled < 2.0 ** -6, torch.tensor(2.0 ** -9, dtype=torch.float64),
                      2.0 ** (torch.floor(torch.log2(scaled.clamp(min=2.0 ** -6))) - 3))
    assert ((q.dequantize().double() - t).abs() <= ulp / 2 * inv).all()


def test_tiny_gpt_mx_forward_cpu():
    """Forward and backward run; the loss is neither the per-tensor model's nor the flag-off model's.  The LayerNorm
    gains span 2^-12 .. 1 across the columns: one scale per tensor flushes the small columns, one per block keeps them."""
    base = dict(block_size=32, vocab_size=100, padded_vocab=128, n_layer=2, n_head=2, n_embd=64)
    models = [build_gpt2(GPTConfig(**base, **kw), seed=0, dtype=torch.float32)
              for kw in (dict(fp8_forward=True, fp8_scaling="mx"), dict(fp8_forward=True), dict())]
    for m in models:
        with torch.no_grad():
            for blk in m.transformer.h:
                blk.ln_1.weight.mul_(2.0 ** -(torch.arange(64) // 5).float())
                blk.ln_2.weight.mul_(2.0 ** -(torch.arange(64) // 5).float())
    torch.manual_seed(3)
    idx, tgt = torch.randint(0, 100, (2, 32)), torch.randint(0, 100, (2, 32))
    mx, tensor, off = (m(idx, tgt) for m in models)
    mx.backward()
    assert torch.isfinite(mx) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in models[0].parameters())
    assert mx.item() != tensor.item() and mx.item() != off.item()
    assert torch.equal(models[0].generate(idx[:, :4], 3, temperature=0.0), models[2].generate(idx[:, :4], 3, temperature=0.0))


def test_bad_fp8_scaling_raises():
    with pytest.raises(ValueError):
        build_gpt2(GPTConfig(n_layer=1, fp8_forward=True, fp8_scaling="block"), seed=0, dtype=torch.float32)
    build_gpt2(GPTConfig(block_size=8, vocab_size=16, padded_vocab=16, n_layer=1, n_head=1, n_embd=32,
                         fp8_scaling="block"), seed=0, dtype=torch.float32)      # not read with fp8_forward off
