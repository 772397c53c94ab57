"""FP8 forward on the GPU: the quantiser bit for bit against ``quantize_reference``, the FP8 GEMM against fp64 on the
dequantised operands, the bf16 backward, graph replay and the model."""
import functools

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import fp8
from pytorch_distributed_example_amd.ops import gemm as G
from pytorch_distributed_example_amd.ops import transformer as T

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
Q_SHAPES = [(1, 16), (3, 192), (257, 768), (1000, 3072)]
Q_FAMILIES = ["normal", "zero", "outlier", "pow2", "edge448"]


def _family(name, shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g)
    if name == "zero":
        t.zero_()
    elif name == "outlier":            # the values around 1e-3 must flush or quantise exactly as the twin's
        t.mul_(1e-3)
        t.view(-1)[t.numel() // 2] = 3e4
    elif name == "pow2":               # amax an exact power of two
        t.clamp_(-3, 3)
        t.view(-1)[-1] = -4.0
    elif name == "edge448":            # amax * s == 448 exactly
        t.clamp_(-1.5, 1.5)
        t.view(-1)[0] = -1.75
    return t.to(BF)


def _same(got, ref):
    return (torch.equal(got.data.view(torch.uint8).cpu(), ref.data.view(torch.uint8))
            and torch.equal(got.scale.cpu(), ref.scale))


@pytest.mark.parametrize("name", Q_FAMILIES)
@pytest.mark.parametrize("shape", Q_SHAPES)
def test_quantize_bit_for_bit(shape, name):
    t = _family(name, shape)
    assert _same(fp8.quantize(t.to(dev)), fp8.quantize_reference(t))


def test_quantize_many_equals_single_calls():
    ts = [_family(n, s, seed=i) for i, (n, s) in enumerate(zip(Q_FAMILIES * 14, Q_SHAPES * 18))]   # 70: two chunks
    many = fp8.quantize_many([t.to(dev) for t in ts])
    for t, q in zip(ts, many):
        assert q.data.shape == t.shape and _same(q, fp8.quantize_reference(t))
    again = fp8.quantize_many([t.to(dev) for t in ts[:3]])          # the workspace was re-armed
    assert all(_same(a, fp8.quantize_reference(t)) for a, t in zip(again, ts))


def test_quantize_contract():
    for bad in (torch.zeros(4, 24, device=dev, dtype=BF), torch.zeros(4, 32, device=dev),
                torch.zeros(32, 32, device=dev, dtype=BF).t()):
        with pytest.raises(NotImplementedError):
            fp8.quantize(bad)


@functools.lru_cache(maxsize=None)
def _gemm_case(M, N, K, outlier):
    """Operands, their GPU quantisation, and in float64 on the dequantised operands: x w^T and sum |x w|."""
    x, w = _family("normal", (M, K), 1), (0.05 * _family("normal", (N, K), 2).float()).to(BF)
    if outlier:
        x.view(-1)[x.numel() // 3] = 300.0
    b = _family("normal", (N,), 3)
    xq, wq = fp8.quantize(x.to(dev)), fp8.quantize(w.to(dev))
    xd, wd = xq.dequantize().double().cpu(), wq.dequantize().double().cpu()
    return xq, wq, b, xd @ wd.t(), xd.abs() @ wd.abs().t()


@pytest.mark.parametrize("outlier", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,N,K", [(8, 8, 64), (16, 16, 128), (257, 264, 192), (300, 776, 832), (512, 2304, 768),
                                   (512, 768, 3072)])
def test_gemm_fp8_against_fp64(M, N, K, bias, outlier):
    """|y - ref| <= 2^-8 |ref| (bf16's half ulp) + K 2^-22 sum_k |xq wq| / (sx sw) (the fp32 accumulation bound
    K 2^-24 sum |a b| times 4 for the MFMA's unspecified internal order); both terms derived, not measured."""
    xq, wq, b, ref, sabs = _gemm_case(M, N, K, outlier)
    y = fp8.fprop(xq, wq, b.to(dev) if bias else None)
    ref = ref + b.double() if bias else ref
    err = (y.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -22 * sabs
    print(f"worst error / bound: {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert y.dtype == BF and y.shape == (M, N) and (err <= bound).all()


@pytest.mark.parametrize("M,N,K", [(257, 264, 192), (512, 3072, 768)])
def test_gemm_fp8_gelu(M, N, K):
    """gelu(pre) and gelu'(pre) to the tolerance tests/test_gemm_gpu.py holds gemm.fprop(gelu=True) to."""
    xq, wq, b, ref, _ = _gemm_case(M, N, K, False)
    act, dgelu = fp8.fprop(xq, wq, b.to(dev), gelu=True)
    rp = (ref + b.double()).requires_grad_()
    want = F.gelu(rp, approximate="tanh")
    want.backward(torch.ones_like(want))
    rel = lambda a, r: ((a.double().cpu() - r).abs().max() / r.abs().max()).item()
    assert rel(act, want.detach()) < 2e-2 and rel(dgelu, rp.grad) < 2e-2


def _operands(M=300, C=128, Nf=512):
    mk = lambda shape, seed, scale=1.0: (scale * _family("normal", shape, seed).float()).to(dev, BF).requires_grad_()
    return mk((M, C), 4), mk((Nf, C), 5, 0.05), mk((Nf,), 6), mk((C, Nf), 7, 0.05), mk((C,), 8)


def test_linear_fp8_backward_is_the_bf16_ops():
    x, w, b, _, _ = _operands()
    dy = _family("normal", (300, 512), 9).to(dev)
    got = torch.autograd.grad(fp8.linear_fp8(x, w, b), (x, w, b), dy)
    ref = torch.autograd.grad(T.linear(x, w, b), (x, w, b), dy)
    assert all(torch.equal(g, r) for g, r in zip(got, ref))
    pre = torch.autograd.grad(fp8.linear_fp8(x, w, b, fp8.quantize(w)), (x, w, b), dy)    # pre-quantised weight
    assert all(torch.equal(g, r) for g, r in zip(pre, ref))


def test_mlp_fp8_backward_is_the_bf16_ops():
    """``MLPFn``'s backward calls on the FP8 forward's saved gelu(pre) and gelu'(pre)."""
    x, w_fc, b_fc, w_proj, b_proj = _operands()
    dy = _family("normal", (300, 128), 10).to(dev)
    y = fp8.mlp_fp8(x, w_fc, b_fc, w_proj, b_proj)
    got = torch.autograd.grad(y, (x, w_fc, b_fc, w_proj, b_proj), dy)
    act, dgelu = fp8.fprop(fp8.quantize(x.detach()), fp8.quantize(w_fc), b_fc.detach(), gelu=True)
    assert torch.equal(y, fp8.fprop(fp8.quantize(act), fp8.quantize(w_proj), b_proj.detach()))
    dw_proj, db_proj = G.wgrad(dy, act, want_db=True)
    dpre = G.dgrad(dy, w_proj.detach(), dgelu=dgelu)
    dw_fc, db_fc = G.wgrad(dpre, x.detach(), want_db=True)
    ref = (G.dgrad(dpre, w_fc.detach()), dw_fc, db_fc, dw_proj, db_proj)
    assert all(torch.equal(g, r) for g, r in zip(got, ref))


def test_graph_replay_follows_the_data():
    """A scale read on the host or frozen into a launch would replay the capture-time scale."""
    x, w, b, _, _ = _operands()
    xs, ws = x.detach().clone(), w.detach().clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        fp8.linear_fp8(xs, ws, b)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        ys = fp8.linear_fp8(xs, ws, b)
    for fx, fw in ((1000.0, 1000.0), (1e-3, 1.0), (1.0, 1000.0)):
        xs.copy_(x.detach() * fx)
        ws.copy_(w.detach() * fw)
        graph.replay()
        with torch.no_grad():
            eager = fp8.linear_fp8(xs, ws, b)
        assert torch.equal(ys, eager) and torch.isfinite(ys.float()).all()


def _twin_cfg(**kw):
    return GPTConfig(block_size=128, vocab_size=1000, padded_vocab=1024, n_layer=4, n_head=2, n_embd=128, **kw)


def test_gpt2_fp8_forward_matches_cpu_twin():
    """The bounds of tests/test_transformer_gpu.py's bf16 parity test (loss within 1e-2, every gradient's cosine
    >= 0.99), GPU bf16 against the CPU fp32 twin, both with ``fp8_forward=True``."""
    g, c = build_gpt2(_twin_cfg(fp8_forward=True), seed=0, device=dev), build_gpt2(_twin_cfg(fp8_forward=True), seed=0,
                                                                                   dtype=torch.float32)
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


def test_gpt2_fp8_forward_off_is_the_model_without_the_field():
    a, b = build_gpt2(_twin_cfg(), seed=0, device=dev), build_gpt2(_twin_cfg(fp8_forward=False), seed=0, device=dev)
    on = build_gpt2(_twin_cfg(fp8_forward=True), seed=0, device=dev)
    torch.manual_seed(6)
    idx, tgt = torch.randint(0, 1000, (2, 128), device=dev), torch.randint(0, 1000, (2, 128), device=dev)
    la, lb, lo = a(idx, tgt), b(idx, tgt), on(idx, tgt)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))
    assert not torch.equal(lo, la)
