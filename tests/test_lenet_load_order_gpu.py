"""Direct checks of the kernels whose load order the step's latency hangs on: ``lenet_fc1_fwd``
(one load batch, unmasked operands), ``lenet_fc_bwd`` (all three roles, one launch and split) and
the fold blocks of ``adam_flat`` / ``sgd_flat``.  References are fp64 on the CPU; every call is
repeated on the same inputs and must reproduce its first result bit for bit (no atomics, fixed
summation order)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCHES = [1, 15, 16, 17, 128]       # ragged / full last m-tile, one block row and several
PAD_ROWS = 16                        # sentinel rows behind the batch


def _close(a, b, rtol, atol, what):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= atol + rtol * scale, f"{what}: max abs err {err:.3e} (ref scale {scale:.3e})"


def _same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: not bit-identical"


def _kernels():
    from pytorch_distributed_example_amd._ext import kernels
    return kernels()


@functools.lru_cache(maxsize=None)
def _fc_weights():
    g = torch.Generator().manual_seed(7)
    W1 = torch.randn(500, 800, generator=g) * 0.05
    b1 = torch.randn(500, generator=g) * 0.1
    return W1, b1


@functools.lru_cache(maxsize=None)
def _fc_case(B):
    """Inputs and fp64 references for batch B (computed once, never modified)."""
    g = torch.Generator().manual_seed(100 + B)
    W1, b1 = _fc_weights()
    P2 = torch.randn(B, 800, generator=g).clamp_min(0.0)         # pooled ReLU output: about half zeros
    H1 = torch.randn(B, 500, generator=g).clamp_min(0.0)
    dZ1 = torch.randn(B, 500, generator=g) / B
    dZ2 = torch.randn(B, 10, generator=g) / B
    d = lambda x: x.double()
    ref = {
        "H1": torch.relu(d(P2) @ d(W1).t() + d(b1)),
        "dP2m": (d(dZ1) @ d(W1)) * (P2 > 0),
        "gW1": d(dZ1).t() @ d(P2),
        "gb1": d(dZ1).sum(0),
        "gW2": d(dZ2).t() @ d(H1),
        "gb2": d(dZ2).sum(0),
    }
    return dict(P2=P2, H1=H1, dZ1=dZ1, dZ2=dZ2), ref


@pytest.mark.parametrize("B", BATCHES)
def test_fc1_fwd_direct(B):
    K = _kernels()
    inp, ref = _fc_case(B)
    W1, b1 = (x.to(DEV) for x in _fc_weights())
    P2 = inp["P2"].to(DEV)
    ctr = torch.tensor([5, 11], dtype=torch.int64, device=DEV)
    outs = []
    for call in range(2):
        H1 = torch.full((B + PAD_ROWS, 500), float("nan"), device=DEV)
        K.lenet_fc1_fwd(P2, B, W1, b1, H1, ctr)
        torch.cuda.synchronize()
        assert ctr.tolist() == [6 + call, 12 + call], f"counters after call {call + 1}: {ctr.tolist()}"
        assert torch.isfinite(H1[:B]).all(), "rows < B must be written"
        assert torch.isnan(H1[B:]).all(), "rows >= B must stay untouched"
        outs.append(H1)
    _close(outs[0][:B], ref["H1"], 1e-5, 1e-5, f"H1 B={B}")
    _same_bits(outs[0][:B], outs[1][:B], f"H1 B={B} second call")
    # without counters: nothing else changes
    H1 = torch.full((B + PAD_ROWS, 500), float("nan"), device=DEV)
    K.lenet_fc1_fwd(P2, B, W1, b1, H1, None)
    torch.cuda.synchronize()
    _same_bits(H1[:B], outs[0][:B], "H1 without counters")
    assert ctr.tolist() == [7, 13]


def _run_fc_bwd(K, inp, W1, B, parts):
    pad = 64
    out = {
        "dP2m": torch.full((B + PAD_ROWS, 800), float("nan"), device=DEV),
        "gW1": torch.full((400000 + pad,), float("nan"), device=DEV),
        "gb1": torch.full((500 + pad,), float("nan"), device=DEV),
        "gW2": torch.full((5000 + pad,), float("nan"), device=DEV),
        "gb2": torch.full((10 + pad,), float("nan"), device=DEV),
    }
    for part in parts:
        K.lenet_fc_bwd(inp["P2"], inp["H1"], inp["dZ1"], inp["dZ2"], W1, B, out["dP2m"], out["gW1"], out["gb1"],
                       out["gW2"], out["gb2"], None, None, None, None, 0, part)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", BATCHES)
def test_fc_bwd_direct(B):
    K = _kernels()
    cpu, ref = _fc_case(B)
    inp = {k: v.to(DEV) for k, v in cpu.items()}
    W1 = _fc_weights()[0].to(DEV)
    first = _run_fc_bwd(K, inp, W1, B, [0])
    sizes = {"dP2m": B * 800, "gW1": 400000, "gb1": 500, "gW2": 5000, "gb2": 10}
    for name, n in sizes.items():
        flat = first[name].view(-1)
        assert torch.isfinite(flat[:n]).all(), f"{name}: every element must be written"
        assert torch.isnan(flat[n:]).all(), f"{name}: sentinel behind the output was overwritten"
        _close(flat[:n], ref[name].reshape(-1), 2e-4, 1e-6, f"{name} B={B}")
    again = _run_fc_bwd(K, inp, W1, B, [0])
    split = _run_fc_bwd(K, inp, W1, B, [1, 2])
    for name, n in sizes.items():
        _same_bits(first[name].view(-1)[:n], again[name].view(-1)[:n], f"{name} B={B} second call")
        _same_bits(first[name].view(-1)[:n], split[name].view(-1)[:n], f"{name} B={B} part 1 + part 2")
        assert torch.isnan(split[name].view(-1)[n:]).all(), f"{name}: sentinel overwritten by the split launch"


def _opt_reference(kind, p, gs, state, t):
    """One step of the optimizer's arithmetic in fp64 on the folded gradient gs."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32).double().item()   # the kernel's fp32 constants
    if kind == "adam":
        lr, b1, b2, eps = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)
        state["m"] = state["m"] + (gs - state["m"]) * (1 - b1)
        state["v"] = state["v"] * b2 + (1 - b2) * gs * gs
        denom = state["v"].sqrt() / (1 - b2 ** t) ** 0.5 + eps
        return p - (lr / (1 - b1 ** t)) * state["m"] / denom
    lr, mom = f32(1e-2), f32(0.9)
    state["m"] = gs.clone() if t == 1 else mom * state["m"] + gs
    return p - lr * state["m"]


@pytest.mark.parametrize("nrep", [1, 2, 16])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_flat_optimizer_fold_lanes(kind, nrep):
    """[plain 1000][fold: nrep x 320, len 200][plain 200].  stride 320 = 80 float4 x 4 lanes = 320 fold
    lanes: the second fold block is a quarter full; elements 200..319 of the slot have no replicas."""
    K = _kernels()
    off, stride, ln = 1000, 320, 200
    n = off + nrep * stride + 200
    gen = torch.Generator().manual_seed(3 * nrep + (kind == "sgd"))
    canon = torch.ones(n, dtype=torch.bool)
    canon[off + stride:off + nrep * stride] = False
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(2)]
    fold = dict(fold_off=off, fold_len=ln, fold_nrep=nrep, fold_stride=stride) if nrep > 1 else {}

    def run():
        p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        step = torch.zeros(1, device=DEV, dtype=torch.int64)
        arrive = torch.zeros(1, device=DEV, dtype=torch.int32)
        gout = []
        for g in grads:
            gd = g.to(DEV)
            if kind == "adam":
                K.adam_flat(p, gd, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, 1.0, step, arrive, 1, **fold)
            else:
                K.sgd_flat(p, gd, m, 1e-2, 0.9, 0.0, 0.0, False, 1.0, step, arrive, 1, **fold)
            gout.append(gd)
        torch.cuda.synchronize()
        assert int(step.item()) == len(grads) and int(arrive.item()) == 0
        return p, m, v, gout

    pref = p0.double()
    state = {"m": torch.zeros(n, dtype=torch.float64), "v": torch.zeros(n, dtype=torch.float64)}
    gsums = []
    for t, g in enumerate(grads, 1):
        gs = g.double()
        for r in range(1, nrep):                                    # replica order
            gs[off:off + ln] += g.double()[off + r * stride:off + r * stride + ln]
        gsums.append(gs)
        pref = _opt_reference(kind, pref, gs, state, t)
    p, m, v, gout = run()
    for t, (gd, gs, g) in enumerate(zip(gout, gsums, grads)):
        _close(gd.cpu()[canon], gs[canon], 1e-6, 1e-6, f"folded grad step {t}")
        assert torch.equal(gd.cpu()[~canon], g[~canon]), f"replica storage step {t}"
    _close(p.cpu()[canon], pref[canon], 0, 3e-6, f"{kind} params nrep={nrep}")
    assert torch.equal(p.cpu()[~canon], p0[~canon]), "replica params untouched"
    _close(m.cpu()[canon], state["m"][canon], 1e-6, 1e-6, f"{kind} first moment / momentum buffer")
    if kind == "adam":
        _close(v.cpu()[canon], state["v"][canon], 1e-6, 1e-9, "adam second moment")
    p2, m2, v2, gout2 = run()
    _same_bits(p, p2, "params, second run")
    _same_bits(m, m2, "moment, second run")
    _same_bits(v, v2, "second moment, second run")
    for a, b in zip(gout, gout2):
        _same_bits(a, b, "folded gradient, second run")
