"""MXFP8 forward on the GPU: every quantising kernel bit for bit against ``quantize_mx_reference``, the block-scaled GEMM
against fp64 on the dequantised operands, the bf16 backward, graph replay and the model."""
import functools

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import fp8
from pytorch_distributed_example_amd.ops import gemm as G
from pytorch_distributed_example_amd.ops import transformer as T
from pytorch_distributed_example_amd.ops.rng import DeviceRNG

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
Q_SHAPES = [(1, 32), (3, 96), (257, 768), (5, 3072)]
Q_FAMILIES = ["normal", "zero", "outlier", "pow2", "m1.75", "m1.875", "2^127", "2^-125"]


def _family(name, shape, seed=0, scale=1.0):
    """bf16 values in blocks of 32; block g of row r is multiplied by 2^((3 r + 5 g) % 11 - 5), so every block's scale
    differs from its row neighbours' and from the same block one row down."""
    g = torch.Generator().manual_seed(seed)
    t = (scale * torch.randn(shape, generator=g)).unflatten(-1, (-1, 32))
    r, b = torch.arange(t[..., 0, 0].numel()).view(*t.shape[:-2], 1), torch.arange(t.shape[-2])
    ramp = (2.0 ** ((3 * r + 5 * b) % 11 - 5)).unsqueeze(-1)
    if name == "zero":                 # a zero block (of both signs) between non-zero blocks
        t[..., 1::3, :] = 0.0
        t[..., 1::3, ::2] = -0.0
    elif name == "outlier":            # one per row; the values around 1e-3 flush or quantise exactly as the twin's
        t.mul_(1e-3)
        t[..., 0, 7] = 3e4
    elif name == "pow2":               # amax an exact power of two
        t.clamp_(-3, 3)[..., 5] = -4.0
    elif name == "m1.75":              # amax * 2^k == 448 exactly
        t.clamp_(-1.5, 1.5)[..., 0] = -1.75
    elif name == "m1.875":             # the other branch of the rule
        t.clamp_(-1.5, 1.5)[..., 31] = 1.875
    elif name in ("2^127", "2^-125"):  # the largest block scale; the k <= 127 clamp
        t.clamp_(-0.9, 0.9)[..., 3] = 1.0
        ramp = torch.tensor(2.0 ** 127 if name == "2^127" else 2.0 ** -125)
    return (t * ramp).flatten(-2).to(BF)


def _same(got, ref):
    return (got.data.shape == ref.data.shape and got.scale.dtype == torch.uint8
            and torch.equal(got.data.view(torch.uint8).cpu(), ref.data.view(torch.uint8))
            and torch.equal(got.scale.cpu(), ref.scale))


@pytest.mark.parametrize("name", Q_FAMILIES)
@pytest.mark.parametrize("shape", Q_SHAPES)
def test_quantize_mx_bit_for_bit(shape, name):
    t = _family(name, shape)
    assert _same(fp8.quantize_mx(t.to(dev)), fp8.quantize_mx_reference(t))


def test_quantize_mx_many_equals_single_calls():
    ts = [_family(n, s, seed=i) for i, (n, s) in enumerate(zip(Q_FAMILIES * 9, Q_SHAPES * 18)) if i < 70]   # two chunks
    many = fp8.quantize_mx_many([t.to(dev) for t in ts])
    assert len(many) == 70 and all(_same(q, fp8.quantize_mx_reference(t)) for t, q in zip(ts, many))


@functools.lru_cache(maxsize=None)
def _gemm_case(M, N, K):
    """Operands, their GPU quantisation, and in float64 on the dequantised operands: x w^T and sum |x w|."""
    x, w, b = _family("normal", (M, K), 1), _family("normal", (N, K), 2, 0.05), _family("normal", (1, 32 * N), 3)[0, :N]
    xq, wq = fp8.quantize_mx(x.to(dev)), fp8.quantize_mx(w.to(dev))
    xd, wd = xq.dequantize().double(), wq.dequantize().double()
    return xq, wq, b, xd @ wd.t(), xd.abs() @ wd.abs().t()


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,N,K", [(8, 8, 128), (40, 72, 128), (257, 264, 256), (300, 776, 896), (512, 2304, 768),
                                   (512, 768, 3072)])
def test_gemm_mxfp8_against_fp64(M, N, K, bias):
    """|y - ref| <= 2^-8 |ref| (bf16's half ulp) + K 2^-22 sum_k |xd wd| (the fp32 accumulation bound K 2^-24 sum |a b|
    times 4 for the MFMA's unspecified internal order); both terms derived, not measured.  A scale applied to the wrong
    block or row is off by a factor of at least 2 in that block's term."""
    xq, wq, b, ref, sabs = _gemm_case(M, N, K)
    y = fp8.fprop_mx(xq, wq, b.to(dev) if bias else None)
    ref = ref + b.double() if bias else ref
    err = (y.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -22 * sabs
    print(f"worst error / bound: {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert y.dtype == BF and y.shape == (M, N) and (err <= bound).all()


@pytest.mark.parametrize("M,N,K", [(257, 288, 256), (512, 3072, 768)])
def test_gemm_mxfp8_gelu_act_mx(M, N, K):
    """gelu(pre) and gelu'(pre) to the tolerance tests/test_fp8_gpu.py holds the pair to; the epilogue's MxTensor is the
    quantisation of the activation the same launch stored."""
    xq, wq, b, ref, _ = _gemm_case(M, N, K)
    act, dgelu, aq = fp8.fprop_mx(xq, wq, b.to(dev), gelu=True, act_mx=True)
    rp = (ref + b.double()).requires_grad_()
    want = F.gelu(rp, approximate="tanh")
    want.backward(torch.ones_like(want))
    rel = lambda a, r: ((a.double().cpu() - r).abs().max() / r.abs().max()).item()
    assert rel(act, want.detach()) < 2e-2 and rel(dgelu, rp.grad) < 2e-2
    assert _same(aq, fp8.quantize_mx_reference(act.cpu()))
    plain = fp8.fprop_mx(xq, wq, b.to(dev), gelu=True)
    assert torch.equal(plain[0], act) and torch.equal(plain[1], dgelu)


def test_gemm_mxfp8_contract():
    q = lambda r, c: fp8.quantize_mx(torch.ones(r, c, device=dev, dtype=BF))
    for xq, wq, kw in ((q(8, 192), q(8, 192), {}), (q(8, 128), q(12, 128), {}), (q(8, 128), q(8, 128), {"act_mx": True}),
                       (q(8, 128), q(8, 128), {"gelu": True, "act_mx": True})):
        with pytest.raises(ValueError):
            fp8.fprop_mx(xq, wq, **kw)


@pytest.mark.parametrize("form", ["plain", "add", "drop"])
@pytest.mark.parametrize("N,C", [(5, 32), (7, 768), (6, 1056), (3, 2048)])
def test_layer_norm_mx_out(N, C, form):
    """The MxTensor is the quantisation of the returned h; every other output, and (through the saved mean and rstd)
    every gradient, is the call's without the flag."""
    mk = lambda shape, seed, name="normal": _family(name, shape, seed).to(dev).requires_grad_()
    x, d, w, b = mk((N, C), 1, "outlier"), mk((N, C), 2), mk((1, C), 3)[0], mk((1, C), 4)[0]
    if form == "plain":
        call = lambda **kw: T.layer_norm_residual(x, w, b, **kw)
    elif form == "add":
        call = lambda **kw: T.add_layer_norm_residual(x, d, w, b, **kw)
    else:
        snap = DeviceRNG(7, 0, device=dev).next()
        call = lambda **kw: T.add_dropout_layer_norm_residual(x, d, w, b, 1e-5, 0.25, snap, 3, **kw)
    s0, h0 = call()
    s1, h1, hq = call(mx_out=True)
    assert torch.equal(s0, s1) and torch.equal(h0, h1) and _same(hq, fp8.quantize_mx_reference(h1.detach().cpu()))
    ins = (x, w, b) if form == "plain" else (x, d, w, b)
    dy = _family("normal", (N, C), 5).to(dev)
    for g0, g1 in zip(torch.autograd.grad((s0, h0), ins, (dy, dy)), torch.autograd.grad((s1, h1), ins, (dy, dy))):
        assert torch.equal(g0, g1)
    y, yq = T.layer_norm(x, w, b, mx_out=True)
    assert torch.equal(y, T.layer_norm(x, w, b)) and _same(yq, fp8.quantize_mx_reference(y.detach().cpu()))


def _operands(M=300, C=128, Nf=512):
    mk = lambda shape, seed, scale=1.0: _family("normal", shape, seed, scale).to(dev).requires_grad_()
    return mk((M, C), 4), mk((Nf, C), 5, 0.05), mk((1, Nf), 6)[0], mk((C, Nf), 7, 0.05), mk((1, C), 8)[0]


def test_linear_mx_backward_is_the_bf16_ops():
    x, w, b, _, _ = _operands()
    dy = _family("normal", (300, 512), 9).to(dev)
    ref = torch.autograd.grad(T.linear(x, w, b), (x, w, b), dy)
    y = fp8.linear_mx(x, w, b)
    assert all(torch.equal(g, r) for g, r in zip(torch.autograd.grad(y, (x, w, b), dy), ref))
    pre = fp8.linear_mx(x, w, b, fp8.quantize_mx(w), fp8.quantize_mx(x.detach()))    # pre-quantised operands
    assert torch.equal(pre, y) and all(torch.equal(g, r) for g, r in zip(torch.autograd.grad(pre, (x, w, b), dy), ref))


def test_mlp_mx_backward_is_the_bf16_ops():
    """``MLPFn``'s backward calls on the MX forward's saved gelu(pre) and gelu'(pre)."""
    x, w_fc, b_fc, w_proj, b_proj = _operands()
    dy = _family("normal", (300, 128), 10).to(dev)
    y = fp8.mlp_mx(x, w_fc, b_fc, w_proj, b_proj)
    got = torch.autograd.grad(y, (x, w_fc, b_fc, w_proj, b_proj), dy)
    act, dgelu = fp8.fprop_mx(fp8.quantize_mx(x.detach()), fp8.quantize_mx(w_fc), b_fc.detach(), gelu=True)
    assert torch.equal(y, fp8.fprop_mx(fp8.quantize_mx(act), fp8.quantize_mx(w_proj), b_proj.detach()))
    dw_proj, db_proj = G.wgrad(dy, act, want_db=True)
    dpre = G.dgrad(dy, w_proj.detach(), dgelu=dgelu)
    dw_fc, db_fc = G.wgrad(dpre, x.detach(), want_db=True)
    ref = (G.dgrad(dpre, w_fc.detach()), dw_fc, db_fc, dw_proj, db_proj)
    assert all(torch.equal(g, r) for g, r in zip(got, ref))


def test_graph_replay_follows_the_data():
    """Captured on its first call (no workspace to create); the scales are device data, so a replay follows them."""
    x, w, b, _, _ = _operands()
    xs, ws = x.detach().clone(), w.detach().clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        ys = fp8.linear_mx(xs, ws, b)
    for fx, fw in ((1000.0, 1000.0), (1e-3, 1.0), (1.0, 1000.0), (1e-3, 1e-3)):
        xs.copy_(x.detach() * fx)
        ws.copy_(w.detach() * fw)
        graph.replay()
        with torch.no_grad():
            eager = fp8.linear_mx(xs, ws, b)
        assert torch.equal(ys, eager) and torch.isfinite(ys.float()).all()


def _twin_cfg(**kw):
    return GPTConfig(block_size=128, vocab_size=1000, padded_vocab=1024, n_layer=4, n_head=2, n_embd=128, **kw)


def test_gpt2_mx_forward_matches_cpu_twin():
    """The bounds of tests/test_transformer_gpu.py's bf16 parity test (loss within 1e-2, every gradient's cosine
    >= 0.99), GPU bf16 against the CPU fp32 twin, both with ``fp8_scaling="mx"``."""
    kw = dict(fp8_forward=True, fp8_scaling="mx")
    g, c = build_gpt2(_twin_cfg(**kw), seed=0, device=dev), build_gpt2(_twin_cfg(**kw), seed=0, dtype=torch.float32)
    with torch.no_grad():
        for pc, pg in zip(c.parameters(), g.parameters()):
            pc.copy_(pg.float())
    torch.manual_seed(5)
    idx, tgt = torch.randint(0, 1000, (4, 128)), torch.randint(0, 1000, (4, 128))
    lg, lc = g(idx.to(dev), tgt.to(dev)), c(idx, tgt)
    lg.backward()
    lc.backward()
    cos = {n: F.cosine_similarity(pg.grad.float().flatten().cpu(), pc.grad.flatten(), dim=0).item()
           for (n, pg), pc in zip(g.named_parameters(), c.parameters())}
    print(f"loss {lg.item():.5f} vs {lc.item():.5f}; lowest gradient cosine {min(cos.values()):.5f}")
    assert abs(lg.item() - lc.item()) < 1e-2
    assert all(v >= 0.99 for v in cos.values()), {n: v for n, v in cos.items() if not v >= 0.99}


@pytest.mark.parametrize("pdrop", [0.0, 0.1])
def test_gpt2_fp8_scaling_default_is_the_model_without_the_field(pdrop):
    mk = lambda **kw: build_gpt2(_twin_cfg(fp8_forward=True, resid_pdrop=pdrop, **kw), seed=0, device=dev).seed_dropout(3)
    a, b, mx = mk(), mk(fp8_scaling="tensor"), mk(fp8_scaling="mx")
    torch.manual_seed(6)
    idx, tgt = torch.randint(0, 1000, (2, 128), device=dev), torch.randint(0, 1000, (2, 128), device=dev)
    la, lb, lm = a(idx, tgt), b(idx, tgt), mx(idx, tgt)
    la.backward()
    lb.backward()
    lm.backward()
    assert torch.equal(la, lb) and all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))
    assert torch.isfinite(lm) and all(torch.isfinite(p.grad.float()).all() for p in mx.parameters())
