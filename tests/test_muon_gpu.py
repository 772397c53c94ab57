"""Muon on the GPU (csrc/kernels/muon.hip): every stage against fp64 with a derived bound, the whole iteration
against fp64 relative to the CPU twin's own deviation, MuonMaster against the definition, reproducibility, GPT."""
import pytest
import torch

from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.optim import AdamWMaster, LRTable, MuonMaster

pytestmark = pytest.mark.gpu
dev = "cuda"
A_, B_, C_ = ops.muon.NS_COEFFS
SHAPES = [[(64, 64)], [(64, 128)], [(192, 320)], [(320, 192)], [(256, 256)], [(128, 128), (128, 320), (128, 192)]]
IDS = ["64x64", "64x128", "192x320", "320x192", "256x256", "group"]


def _inputs(shapes, kind, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * len(shapes) + shapes[0][0] + shapes[0][1])
    xs = [torch.randn(*s, generator=g) for s in shapes]
    if kind == "rowscaled":
        xs = [x * torch.logspace(-3, 0, x.shape[0])[:, None] for x in xs]
    return [x.bfloat16() for x in xs]


def _check(got, x, y, K, alpha=0.0, c=None, beta=1.0):
    """|err| <= 2 K 2^-24 sum |terms| + 2^-8 |ref| + tiny: fp32 accumulation of K exact products (and the fp32 axpy),
    then the one bf16 rounding."""
    x, y = x.double().cpu(), y.double().cpu()
    ref, mag = beta * (x @ y), abs(beta) * (x.abs() @ y.abs())
    if c is not None:
        ref, mag = ref + alpha * c.double().cpu(), mag + abs(alpha) * c.double().cpu().abs()
    err = (got.double().cpu() - ref).abs()
    bound = 2 * K * 2.0 ** -24 * mag + 2.0 ** -8 * ref.abs() + 1e-30
    print("max err / bound", (err / bound).max().item())
    assert (err <= bound).all(), (err / bound).max().item()


@pytest.mark.parametrize("kind", ["gauss", "rowscaled"])
@pytest.mark.parametrize("shapes", SHAPES, ids=IDS)
def test_stages_against_fp64(shapes, kind):
    xs = [x.to(dev) for x in _inputs(shapes, kind)]
    xs = [x / x.float().norm() for x in xs]                          # the iteration's operating range
    As = ops.muon.gram(xs)                                           # A = X X^T
    Bs = ops.muon.gram(As, As, B_, C_)                               # B = b A + c A A
    Ys = ops.muon.apply_sym(Bs, xs, A_)                              # X' = a X + B X
    for x, a, b, y in zip(xs, As, Bs, Ys):
        assert torch.equal(a, a.t()) and torch.equal(b, b.t())
        _check(a, x, x.t(), x.shape[1])
        _check(b, a, a, a.shape[0], B_, a, C_)
        _check(y, b, x, b.shape[0], A_, x)


@pytest.mark.parametrize("kind", ["gauss", "rowscaled"])
@pytest.mark.parametrize("shapes", SHAPES, ids=IDS)
def test_iteration_against_fp64(shapes, kind):
    """Not derivable: the GPU may deviate from fp64 at most twice as far as the twin does on the same input (the only
    difference between the two is fp32 accumulation order flipping single bf16 roundings)."""
    xs = _inputs(shapes, kind, seed=1)
    out = ops.newton_schulz([x.to(dev) for x in xs])
    for x, o in zip(xs, out):
        ref = ops.newton_schulz_reference(x, emulate=False)
        twin = (ops.newton_schulz_reference(x).double() - ref).norm() / ref.norm()
        gpu = (o.double().cpu() - ref).norm() / ref.norm()
        print(tuple(x.shape), kind, "twin", twin.item(), "gpu", gpu.item(), "ratio", (gpu / twin).item())
        assert o.shape == x.shape and gpu <= 2 * twin, (gpu.item(), twin.item())


def test_limits():
    for bad in (torch.zeros(64, 96), torch.zeros(64), torch.zeros(32, 64)):
        with pytest.raises(ValueError):
            ops.newton_schulz([bad.bfloat16().to(dev)])
    with pytest.raises(ValueError):
        ops.newton_schulz([torch.zeros(64, 64, device=dev)])


MATS = [(64, 128), (192, 64), (128, 128)]


def _muon_run(steps, capturable=False, graph=False, lrs=None, wd=0.1):
    g = torch.Generator().manual_seed(5)
    ws = [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).bfloat16().to(dev)) for s in MATS]
    grads = [[torch.randn(*s, generator=g).bfloat16() for s in MATS] for _ in range(steps)]
    opt = MuonMaster(ws, lr=0.02, momentum=0.9, weight_decay=wd, grad_scale=0.5, capturable=capturable)
    if lrs is not None:
        LRTable(opt, lrs)
    opt.state_tensors()                                              # the state exists before a capture

    def one(gs):
        for w, gr in zip(ws, gs):
            w.grad.copy_(gr)                                         # the flat gradient views
        opt.step()

    if graph:
        cg = torch.cuda.CUDAGraph()
        stage = [torch.zeros_like(w) for w in ws]
        with torch.cuda.graph(cg):
            for w, s in zip(ws, stage):
                w.grad.copy_(s)
            opt.step()
        for gs in grads:
            for s, gr in zip(stage, gs):
                s.copy_(gr)
            cg.replay()
    else:
        for gs in grads:
            one(gs)
    torch.cuda.synchronize()
    return ws, grads, opt


def test_muon_master_steps_against_definition():
    lr, mu, wd, steps = 0.02, 0.9, 0.1, 2
    ws0 = _muon_run(0)[0]
    ws, grads, opt = _muon_run(steps)
    for i, (w0, w) in enumerate(zip(ws0, ws)):
        R, C = w.shape
        Wm, M = w0.detach().double().cpu(), torch.zeros(R, C, dtype=torch.float64)
        slack = 0.0
        for t in range(steps):
            gr = grads[t][i].double() * 0.5
            M = mu * M + gr
            U = gr + mu * M
            O, ref = ops.newton_schulz_reference(U), ops.newton_schulz_reference(U, emulate=False)
            Wm = Wm * (1 - lr * wd) - lr * max(1.0, R / C) ** 0.5 * O.double()
            # the kernels' O may sit as far from the twin's as twice the twin sits from fp64 (see the iteration test)
            slack += lr * max(1.0, R / C) ** 0.5 * 3 * (O.double() - ref).norm().item()
        st = opt.state[w]
        assert torch.allclose(st["momentum_buffer"].double().cpu(), M, rtol=1e-6, atol=1e-7)
        d = (st["master"].double().cpu() - Wm).norm().item()
        print(tuple(w.shape), "master diff", d, "allowed", slack)
        assert d <= slack + 1e-6 * Wm.norm().item()
        assert torch.equal(w.detach(), st["master"].bfloat16())
        assert float(st["step"]) == steps


def test_bit_reproducible_and_graph_replay():
    lrs = [0.02, 0.01, 0.005]
    runs = [_muon_run(3, capturable=c, graph=g, lrs=lrs) for c, g in ((False, False), (False, False), (True, True))]
    for ws, _, opt in runs[1:]:
        for a, b in zip(runs[0][0], ws):
            assert torch.equal(a, b)
            assert torch.equal(runs[0][2].state[a]["master"], opt.state[b]["master"])
            assert torch.equal(runs[0][2].state[a]["momentum_buffer"], opt.state[b]["momentum_buffer"])
    assert runs[2][2].lr_step_count() == 3
    other = _muon_run(3, lrs=[0.02, 0.02, 0.02])[0]                 # the table is read: another schedule, other weights
    assert not torch.equal(other[0], runs[0][0][0])


def test_gpt_trains_with_muon_and_adamw():
    cfg = GPTConfig(block_size=128, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128)
    m = build_gpt2(cfg, seed=1, device=dev)
    mats, rest = m.muon_groups()
    muon, adam = MuonMaster(mats, lr=0.02, weight_decay=0.01), AdamWMaster(rest, lr=3e-3, weight_decay=0.0)
    torch.manual_seed(8)
    idx = torch.randint(0, cfg.vocab_size, (4, 128), device=dev)
    losses = []
    for _ in range(12):
        muon.zero_grad()
        adam.zero_grad()
        loss = m(idx, torch.roll(idx, -1, 1))
        loss.backward()
        muon.step()
        adam.step()
        losses.append(loss.item())
    print(losses)
    assert losses[-1] < 0.7 * losses[0], losses
    sd = muon.state_dict()
    fresh = MuonMaster(mats, lr=0.02, weight_decay=0.01)
    fresh.load_state_dict(sd)
    for p in mats:
        for k in ("master", "momentum_buffer"):
            assert torch.equal(fresh.state[p][k], muon.state[p][k])
    assert fresh.lr_step_count() == 12
