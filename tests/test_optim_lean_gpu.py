"""The lean flat optimizers (``adam_flat`` without a peer, ``sgd_flat``): fold blocks first, arguments
worked out on the host, the first iteration's loads ahead of the wait for the step counter.

Adam: the lean kernel against the general one (the kernel of the fused all-reduce routes, forced for
a peer-less call with ``optim_force_general``) bit for bit -- parameters, moments, gradients, the
packed conv2 weight, counters and the arrival word.  SGD has one body, so it is compared against an
fp64 reference with the tolerances ``tests/test_lenet_load_order_gpu.py`` uses for its optimizer
cases (parameters 3e-6 absolute, buffers / folded gradients 1e-6 relative to the largest reference
value + 1e-6).  NaN sentinels sit behind every buffer and must survive; every call repeated on the
same inputs must reproduce its first result bit for bit."""
import contextlib
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64                                             # sentinel floats behind every buffer
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
SGD = dict(lr=1e-2, momentum=0.9)
SIZES = [4, 1020, 1024, 1028, 4 * (3 * 256) + 4]     # one float4, block edges, a ragged last block


def _kernels():
    from pytorch_distributed_example_amd._ext import kernels
    return kernels()


@contextlib.contextmanager
def _general(K, on):
    K.optim_force_general(bool(on))
    try:
        yield
    finally:
        K.optim_force_general(False)


def _f32(x):
    return torch.tensor(x, dtype=torch.float32).double().item()


def _bits(x):
    return x.view(torch.int32)


WP_FLOATS = 2 * 72 * 256                             # the packed conv2 weight of the conv forward


def _image(cpu):
    """p | g | m | v with NaN sentinels behind each, uploaded once per input set."""
    if "_image" not in cpu:
        n = cpu["p"].numel()
        img = torch.full((4, n + PAD), float("nan"))
        for k, name in enumerate("pgmv"):
            img[k, :n] = cpu[name]
        cpu["_image"] = img.view(-1).to(DEV)
    return cpu["_image"]


class Bufs:
    """p | g | m | v in one allocation, NaN sentinels behind each; the same for the pack destination."""

    def __init__(self, cpu, pack=False):
        self.n = cpu["p"].numel()
        self.all = _image(cpu).clone()
        self.p, self.g, self.m, self.v = (self.view(k) for k in range(4))
        self.pack = None
        if pack:
            self.pack_all = torch.full((WP_FLOATS + PAD,), float("nan"), device=DEV)
            self.pack = self.pack_all[:WP_FLOATS]

    def view(self, k):
        return self.all[k * (self.n + PAD): k * (self.n + PAD) + self.n]

    def sentinels_intact(self):
        pads = self.all.view(4, self.n + PAD)[:, self.n:]
        ok = bool(torch.isnan(pads).all())
        if self.pack is not None:
            ok = ok and bool(torch.isnan(self.pack_all[WP_FLOATS:]).all())
        return ok


def _wp_index(e):
    """csrc/include/pde_lenet.h pde_lenet_wp_index, on an int64 tensor."""
    co, k = e // 500, e % 500
    ci, tap = k // 25, k % 25
    kp = tap * 20 + ci
    s, kq = kp >> 2, kp & 3
    return (co >> 5) * (72 * 256) + ((((co >> 4) & 1) * 4 + kq) * 16 + (co & 15)) * 132 + s


def _inputs(n, seed, zero_state=False):
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m = torch.zeros(n) if zero_state else torch.randn(n, generator=gen)
    v = torch.zeros(n) if zero_state else torch.randn(n, generator=gen).square()
    return dict(p=p, g=g, m=m, v=v)


def _call(K, kind, b, step, arrive, bump, wd=0.0, flag=False, gs=1.0, lr_table=None, **kw):
    if kind == "adam":
        K.adam_flat(b.p, b.g, b.m, b.v, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd, flag, gs, step, arrive,
                    bump, lr_table=lr_table, **kw)
    else:
        K.sgd_flat(b.p, b.g, b.m, SGD["lr"], SGD["momentum"], 0.0, wd, flag, gs, step, arrive, bump,
                   lr_table=lr_table, **kw)


def _counters_after(s0, bump):
    return [s0 + 1, 78] if bump == 2 else [s0, 77]


def _run(K, kind, cpu, s0, bump, general=False, pack=False, **kw):
    b = Bufs(cpu, pack)
    step = torch.tensor([s0, 77], dtype=torch.int64, device=DEV)
    arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
    if pack:
        kw = dict(kw, pack_dst=b.pack, pack_mode=2)
    with _general(K, general):
        _call(K, kind, b, step, arrive, bump, **kw)
    return b, step, arrive


def _sgd_reference(cpu, t, wd, nesterov, gs, lr):
    """torch.optim.SGD's arithmetic in fp64 on the kernel's fp32 constants; returns (p, buf)."""
    mom, wd, gs, lr = _f32(SGD["momentum"]), _f32(wd), _f32(gs), _f32(lr)
    p, b = cpu["p"].double(), cpu["m"].double()
    d = cpu["g"].double() * gs
    if wd != 0.0:
        d = d + wd * p
    b = d.clone() if t == 1 else mom * b + d
    d = d + mom * b if nesterov else b
    return p - lr * d, b


def _close(a, ref, rtol, atol, what):
    a = a.detach().double().cpu()
    err = (a - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= atol + rtol * scale, f"{what}: max abs err {err:.3e} (ref scale {scale:.3e})"


def _matrix():
    """(step counter, bump, lr table, wd, decoupled / nesterov, grad_scale): the full product."""
    tables = [None, [3e-3], [1e-3, 2e-3, 5e-4]]       # none, length 1, length 3 (step 999 is past its end)
    return itertools.product([0, 1, 999], [-1, 0, 2], tables, [0.0, 0.01], [False, True], [1.0, 0.125])


@pytest.mark.parametrize("n", SIZES)
def test_adam_lean_equals_general(n):
    K = _kernels()
    cpu = _inputs(n, 11 + n)
    for s0, bump, tab, wd, dec, gs in _matrix():
        what = f"n={n} step={s0} bump={bump} table={tab} wd={wd} decoupled={dec} grad_scale={gs}"
        lrt = None if tab is None else torch.tensor(tab, dtype=torch.float32, device=DEV)
        kw = dict(wd=wd, flag=dec, gs=gs, lr_table=lrt)
        gen, gstep, garr = _run(K, "adam", cpu, s0, bump, general=True, **kw)
        lean, lstep, larr = _run(K, "adam", cpu, s0, bump, **kw)
        again, _, _ = _run(K, "adam", cpu, s0, bump, **kw)
        assert torch.equal(_bits(gen.all), _bits(lean.all)), f"{what}: lean differs from general"
        assert torch.equal(_bits(lean.all), _bits(again.all)), f"{what}: second call differs"
        assert lean.sentinels_intact() and gen.sentinels_intact(), f"{what}: sentinel overwritten"
        assert torch.equal(lean.g.cpu(), cpu["g"]), f"{what}: gradient changed without a fold"
        assert lstep.tolist() == gstep.tolist() == _counters_after(s0, bump), f"{what}: counters {lstep.tolist()}"
        assert int(larr.item()) == 0 and int(garr.item()) == 0, f"{what}: arrive not back at 0"


@pytest.mark.parametrize("n", SIZES)
def test_sgd_matrix_against_fp64(n):
    K = _kernels()
    cpu = _inputs(n, 23 + n)
    for s0, bump, tab, wd, nest, gs in _matrix():
        what = f"n={n} step={s0} bump={bump} table={tab} wd={wd} nesterov={nest} grad_scale={gs}"
        lrt = None if tab is None else torch.tensor(tab, dtype=torch.float32, device=DEV)
        kw = dict(wd=wd, flag=nest, gs=gs, lr_table=lrt)
        t = s0 if bump < 0 else s0 + 1
        lr = SGD["lr"] if tab is None else tab[max(0, min(t - 1, len(tab) - 1))]
        pref, bref = _sgd_reference(cpu, t, wd, nest, gs, lr)
        out, step, arrive = _run(K, "sgd", cpu, s0, bump, **kw)
        again, _, _ = _run(K, "sgd", cpu, s0, bump, **kw)
        _close(out.p, pref, 0, 3e-6, f"{what}: params")
        _close(out.m, bref, 1e-6, 1e-6, f"{what}: momentum buffer")
        assert torch.equal(_bits(out.all), _bits(again.all)), f"{what}: second call differs"
        assert out.sentinels_intact(), f"{what}: sentinel overwritten"
        assert torch.equal(out.g.cpu(), cpu["g"]) and torch.equal(out.v.cpu(), cpu["v"]), f"{what}: g / v changed"
        assert step.tolist() == _counters_after(s0, bump), f"{what}: counters {step.tolist()}"
        assert int(arrive.item()) == 0, f"{what}: arrive not back at 0"


# ------------------------------------------------------------------------------------------ folds
def _fold_reference(kind, cpu, ranges, steps):
    """fp64 optimizer steps from zero state on the folded gradients (replica order); ranges =
    [(off, len, nrep, stride)].  Returns (params, m, v, [folded gradient per step], canonical mask)."""
    n = cpu["p"].numel()
    canon = torch.ones(n, dtype=torch.bool)
    for off, ln, nrep, stride in ranges:
        canon[off + stride: off + nrep * stride] = False
    p = cpu["p"].double()
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    folded = []
    for t, g in enumerate(steps, 1):
        gs = g.double()
        for off, ln, nrep, stride in ranges:
            for r in range(1, nrep):
                gs[off:off + ln] += g.double()[off + r * stride: off + r * stride + ln]
        folded.append(gs)
        if kind == "adam":
            lr, b1, b2, eps = (_f32(ADAM[k]) for k in ("lr", "b1", "b2", "eps"))
            m = m + (gs - m) * (1 - b1)
            v = v * b2 + (1 - b2) * gs * gs
            p = p - (lr / (1 - b1 ** t)) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        else:
            lr, mom = _f32(SGD["lr"]), _f32(SGD["momentum"])
            m = gs.clone() if t == 1 else mom * m + gs
            p = p - lr * m
    return p, m, v, folded, canon


def _fold_steps(K, kind, cpu, grads, general, pack_off, **fold):
    """Two optimizer steps from zero state, a fresh gradient buffer per step."""
    b = Bufs(cpu, pack=pack_off >= 0)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
    kw = dict(fold, pack_off=pack_off, pack_dst=b.pack, pack_mode=2) if pack_off >= 0 else dict(fold)
    gout = []
    with _general(K, general):
        for g in grads:
            b.g.copy_(g)
            _call(K, kind, b, step, arrive, 1, **kw)
            gout.append(b.g.clone())
    assert int(step.item()) == len(grads) and int(arrive.item()) == 0
    assert b.sentinels_intact(), "sentinel overwritten"
    return b, gout


def _check_folds(kind, n, ranges, fold, pack_off, seed):
    K = _kernels()
    gen = torch.Generator().manual_seed(seed)
    cpu = dict(p=torch.randn(n, generator=gen), g=torch.zeros(n), m=torch.zeros(n), v=torch.zeros(n))
    grads = [torch.randn(n, generator=gen) for _ in range(2)]
    pref, mref, vref, folded, canon = _fold_reference(kind, cpu, ranges, grads)
    out, gout = _fold_steps(K, kind, cpu, grads, False, pack_off, **fold)
    for t, (gd, gs, g) in enumerate(zip(gout, folded, grads)):
        _close(gd.cpu()[canon], gs[canon], 1e-6, 1e-6, f"folded grad step {t}")
        assert torch.equal(gd.cpu()[~canon], g[~canon]), f"replica storage step {t}"
    _close(out.p.cpu()[canon], pref[canon], 0, 3e-6, f"{kind} params")
    assert torch.equal(out.p.cpu()[~canon], cpu["p"][~canon]), "replica params untouched"
    _close(out.m.cpu()[canon], mref[canon], 1e-6, 1e-6, f"{kind} first moment / momentum buffer")
    if kind == "adam":
        _close(out.v.cpu()[canon], vref[canon], 1e-6, 1e-9, "adam second moment")
    if pack_off >= 0:                                  # the repacked conv2 weight is the updated parameter
        want = torch.full((WP_FLOATS,), float("nan"))
        want[_wp_index(torch.arange(25000))] = out.p.cpu()[pack_off:pack_off + 25000]
        assert torch.equal(_bits(out.pack.cpu()), _bits(want)), "packed conv2 weight"
    again, gout2 = _fold_steps(K, kind, cpu, grads, False, pack_off, **fold)
    assert torch.equal(_bits(out.all), _bits(again.all)), "second run differs"
    if kind == "adam":
        genl, goutg = _fold_steps(K, kind, cpu, grads, True, pack_off, **fold)
        assert torch.equal(_bits(out.all), _bits(genl.all)), "lean differs from general"
        for a, b in zip(gout, goutg):
            assert torch.equal(_bits(a), _bits(b)), "folded gradient: lean differs from general"
        if pack_off >= 0:
            assert torch.equal(_bits(out.pack_all), _bits(genl.pack_all)), "pack destination: lean differs from general"
    for a, b in zip(gout, gout2):
        assert torch.equal(_bits(a), _bits(b)), "folded gradient, second run"


@pytest.mark.parametrize("nrep", [1, 2, 16])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_fold_conv1_layout(kind, nrep):
    """[plain 1000][fold: nrep x 576, 520 used][plain 200]: the conv1 slot; 576 fold lanes = 2.25 blocks."""
    off, stride, ln = 1000, 576, 520
    n = off + nrep * stride + 200
    fold = dict(fold_off=off, fold_len=ln, fold_nrep=nrep, fold_stride=stride) if nrep > 1 else {}
    _check_folds(kind, n, [(off, ln, nrep, stride)] if nrep > 1 else [], fold, -1, 5 * nrep + (kind == "sgd"))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_fold_engine_layout(kind):
    """The flat layout of the engine's deferred gradient reduction: conv1 replicas 16 x 576, conv2 slabs
    16 x 25088, the conv2 weight repacked for the conv forward."""
    from pytorch_distributed_example_amd.engine import lenet as E
    from pytorch_distributed_example_amd.parallel.flat import FlatLayout

    named = [("conv1.weight", (20, 1, 5, 5)), ("conv1.bias", (20,)), ("conv2.weight", (50, 20, 5, 5)),
             ("conv2.bias", (50,)), ("fc1.weight", (500, 800)), ("fc1.bias", (500,)), ("fc2.weight", (10, 500)),
             ("fc2.bias", (10,))]
    lay = FlatLayout(named, [E.FC_BUCKET, E.CONV_BUCKET + ["conv2.grad_replicas"]],
                     extra_shapes={"conv1.grad_replicas": ((E.C1_NREP - 1) * E.C1_STRIDE,),
                                   "conv2.grad_replicas": ((E.C2_NREP - 1) * E.C2_STRIDE,)})
    c1, c2 = lay.slots["conv1.weight"].offset, lay.slots["conv2.weight"].offset
    assert (E.C1_NREP, E.C1_STRIDE, E.C2_NREP, E.C2_STRIDE) == (16, 576, 16, 25088)
    fold = dict(fold_off=c1, fold_len=E.C1_STRIDE, fold_nrep=E.C1_NREP, fold_stride=E.C1_STRIDE,
                fold2_off=c2, fold2_len=E.C2_STRIDE, fold2_nrep=E.C2_NREP, fold2_stride=E.C2_STRIDE)
    ranges = [(c1, E.C1_STRIDE, E.C1_NREP, E.C1_STRIDE), (c2, E.C2_STRIDE, E.C2_NREP, E.C2_STRIDE)]
    _check_folds(kind, lay.total, ranges, fold, c2, 41 + (kind == "sgd"))


# ------------------------------------------------------------------------------- grid cap, PROF
def test_grid_cap_second_ragged_iteration():
    """More float4s than 2048 blocks x 256 threads: the grid-stride loop runs a second, ragged iteration."""
    K = _kernels()
    n = 4 * (2048 * 256 + 5)
    cpu = _inputs(n, 3)
    gen, _, _ = _run(K, "adam", cpu, 4, 2, general=True)
    lean, step, arrive = _run(K, "adam", cpu, 4, 2)
    again, _, _ = _run(K, "adam", cpu, 4, 2)
    assert torch.equal(_bits(gen.all), _bits(lean.all)), "lean differs from general"
    assert torch.equal(_bits(lean.all), _bits(again.all)), "second call differs"
    assert lean.sentinels_intact() and step.tolist() == [5, 78] and int(arrive.item()) == 0
    assert not torch.equal(lean.p[-20:].cpu(), cpu["p"][-20:]), "the ragged second iteration was not updated"
    pref, bref = _sgd_reference(cpu, 5, 0.0, False, 1.0, SGD["lr"])
    out, _, _ = _run(K, "sgd", cpu, 4, 2)
    _close(out.p, pref, 0, 3e-6, "sgd params")
    _close(out.m, bref, 1e-6, 1e-6, "sgd momentum buffer")
    assert out.sentinels_intact()


def test_prof_instantiation():
    """The phase-stamp instantiation (turned on the way tools/lenet_phases.py does): same results, and
    stamp slots 0 and 1 of every block written."""
    K = _kernels()
    n = SIZES[-1]
    blocks = (n // 4 + 255) // 256
    cpu = _inputs(n, 9)
    plain, _, _ = _run(K, "adam", cpu, 7, 2)
    buf = torch.zeros(6 * 4096 * 8, dtype=torch.int64, device=DEV)
    K.lenet_set_prof(buf)
    try:
        prof, step, arrive = _run(K, "adam", cpu, 7, 2)
        torch.cuda.synchronize()
    finally:
        K.lenet_set_prof(None)
    assert torch.equal(_bits(plain.all), _bits(prof.all)), "results changed with the stamps on"
    assert prof.sentinels_intact() and step.tolist() == [8, 78] and int(arrive.item()) == 0
    stamps = buf.view(6, 4096, 8)[5].cpu()
    assert (stamps[:blocks, :2] > 0).all(), "a block left stamp slot 0 or 1 unwritten"
    assert (stamps[:blocks, 1] >= stamps[:blocks, 0]).all()
    assert (stamps[blocks:] == 0).all() and (stamps[:, 2:] == 0).all(), "stamps outside the launched blocks"
