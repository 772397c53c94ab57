"""GPU numerics of the fused LeNet HIP kernels vs plain PyTorch references (fp64 CPU)."""
import pytest
import torch

from pytorch_distributed_example_amd.models import build_net
from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd.engine import LeNetTrainStep
from reference_impl import torch_twin, ref_step_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batch(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, 28, 28, generator=g)
    y = torch.randint(0, 10, (B,), generator=g)
    return x, y


def _close(a, b, rtol, atol, what):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= atol + rtol * scale, f"{what}: max abs err {err:.3e} (ref scale {scale:.3e})"


def _mostly_close(a, b, mean_tol, max_tol, what):
    """Adam normalises each gradient element (g/sqrt(v)), so elements whose gradient is ~0 can move
    by up to 2*lr on rounding noise alone; compare the bulk tightly and bound the worst case."""
    d = (a.detach().double().cpu() - b.detach().double().cpu()).abs()
    assert d.mean().item() <= mean_tol, f"{what}: mean abs diff {d.mean().item():.3e}"
    assert d.max().item() <= max_tol, f"{what}: max abs diff {d.max().item():.3e}"


@pytest.mark.parametrize("B", [1, 16, 48, 76, 96, 128, 200])
def test_forward_matches_torch(B):
    net = build_net(seed=1, device=DEV)
    ref = torch_twin(net)
    x, y = _batch(B, seed=B)
    with torch.no_grad():
        out = net(x.to(DEV))
        r = ref(x.double())
    _close(out, r, 1e-5, 1e-5, f"logp B={B}")


@pytest.mark.parametrize("B", [1, 32, 76, 128])
def test_backward_matches_torch(B):
    net = build_net(seed=2, device=DEV)
    ref = torch_twin(net)
    x, y = _batch(B, seed=100 + B)
    out = net(x.to(DEV))
    loss = torch.nn.functional.nll_loss(torch.log_softmax(out, 1), y.to(DEV))  # CE(logp) as in the reference
    loss.backward()
    _, rloss, rg = ref_step_grads(ref, x.double(), y)
    _close(loss, rloss, 1e-5, 1e-6, "loss")
    for n, p in net.named_parameters():
        _close(p.grad, rg[n], 2e-4, 1e-6, f"grad {n} B={B}")


@pytest.mark.parametrize("B", [128, 76])
def test_engine_step_grads_and_loss(B):
    net = build_net(seed=3, device=DEV)
    ref = torch_twin(net)
    n = 4 * B + 10
    x, y = _batch(n, seed=7)
    eng = LeNetTrainStep(net, batch_size=B)
    eng.bind_dataset(x.to(DEV), y.to(DEV))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(torch.int32)
    eng.set_epoch_indices(perm)
    eng.step(B)  # batch 0
    torch.cuda.synchronize()
    sel = perm[:B].long()
    _, rloss, rg = ref_step_grads(ref, x[sel].double(), y[sel])
    loss_sum, correct, _ = eng.read_meters()
    _close(torch.tensor(loss_sum / B), rloss, 1e-5, 1e-6, "engine loss")
    for name in rg:
        _close(eng.g[name], rg[name], 2e-4, 1e-6, f"engine grad {name}")


def test_adam_kernel_matches_torch_adam():
    from pytorch_distributed_example_amd._ext import kernels
    K = kernels()
    torch.manual_seed(0)
    n = 4096
    p = torch.randn(n, device=DEV)
    pref = p.detach().clone().cpu().requires_grad_(True)
    opt = torch.optim.Adam([pref], lr=1e-3)
    m = torch.zeros_like(p); v = torch.zeros_like(p)
    step = torch.zeros(1, device=DEV, dtype=torch.int64); arrive = torch.zeros(1, device=DEV, dtype=torch.int32)
    for it in range(5):
        g = torch.randn(n) * (10 ** (it - 2))
        pref.grad = g.clone()
        opt.step()
        K.adam_flat(p, g.to(DEV), m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, 1.0, step, arrive, 1, -1, None)
    torch.cuda.synchronize()
    assert int(step.item()) == 5
    _close(p, pref.detach(), 0, 2e-6, "adam params")


@pytest.mark.parametrize("opt_kind", ["adam", "sgd"])
def test_fused_optimizer_skips_params_without_grad(opt_kind):
    """torch.optim leaves a parameter whose grad is None (and its state) untouched; so must the fused
    flat-buffer optimizer, although its kernel sweeps the whole buffer."""
    from pytorch_distributed_example_amd.optim import SGD, Adam
    torch.manual_seed(5)
    ps = [torch.randn(300, device=DEV, requires_grad=True), torch.randn(64, 5, device=DEV, requires_grad=True)]
    ref = [p.detach().clone().requires_grad_() for p in ps]
    kw = dict(lr=1e-2) if opt_kind == "adam" else dict(lr=0.1, momentum=0.9)
    ours = (Adam if opt_kind == "adam" else SGD)(ps, **kw)
    theirs = (torch.optim.Adam if opt_kind == "adam" else torch.optim.SGD)(ref, foreach=False, **kw)
    for it in range(4):
        used = [0, 1] if it % 2 == 0 else [0]       # parameter 1 gets no gradient on odd steps
        for o in (ours, theirs):
            o.zero_grad(set_to_none=True)
        for i in used:
            g = torch.randn_like(ps[i])
            ps[i].grad = g.clone()
            ref[i].grad = g.clone()
        ours.step()
        theirs.step()
    torch.cuda.synchronize()
    # Adam's bias correction uses the group's shared device step counter, so only the step at which the
    # parameter was last skipped differs (it3 skipped param 1): compare param 0 tightly, param 1 after
    # its last skip has not moved, as torch's has not.
    _close(ps[0], ref[0], 1e-5, 1e-6, f"{opt_kind} used param")
    if opt_kind == "sgd":
        _close(ps[1], ref[1], 1e-5, 1e-6, "sgd skipped param")
    before = ps[1].detach().clone()
    ours.zero_grad(set_to_none=True)
    ps[0].grad = torch.randn_like(ps[0])
    ours.step()
    torch.cuda.synchronize()
    assert torch.equal(ps[1].detach(), before), "a parameter without grad was updated"


@pytest.mark.parametrize("opt_kind", ["adam", "sgd"])
def test_flat_optimizer_folds_replicas(opt_kind):
    """Two folded ranges (replica sets summed by the optimizer's fold blocks, one with a tail past
    ``len`` that has no replicas) plus plain elements on both sides: parameters match torch's
    optimizer fed the summed gradient, the canonical gradient slot holds that sum, and the replica
    storage is left alone."""
    from pytorch_distributed_example_amd._ext import kernels
    K = kernels()
    torch.manual_seed(1)
    # [plain 1000][fold A: 3 reps x 64 (len 48)][plain 36][fold B: 16 reps x 1024][plain 200]
    a_off, a_nrep, a_stride, a_len = 1000, 3, 64, 48
    b_off, b_nrep, b_stride = a_off + a_nrep * a_stride + 36, 16, 1024
    n = b_off + b_nrep * b_stride + 200
    p = torch.randn(n, device=DEV)
    p0 = p.cpu()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    canon = torch.zeros(n, dtype=torch.bool)
    canon[:a_off] = True
    canon[a_off:a_off + a_stride] = True
    canon[a_off + a_nrep * a_stride:b_off] = True
    canon[b_off:b_off + b_stride] = True
    canon[b_off + b_nrep * b_stride:] = True
    pref = p.detach().cpu()[canon].clone().requires_grad_(True)
    opt = (torch.optim.Adam([pref], lr=1e-3) if opt_kind == "adam"
           else torch.optim.SGD([pref], lr=1e-2, momentum=0.9))
    step = torch.zeros(1, device=DEV, dtype=torch.int64)
    arrive = torch.zeros(1, device=DEV, dtype=torch.int32)
    for it in range(4):
        g = torch.randn(n)
        gs = g.clone()
        for off, nrep, stride, ln in ((a_off, a_nrep, a_stride, a_len), (b_off, b_nrep, b_stride, b_stride)):
            for r in range(1, nrep):
                gs[off:off + ln] += g[off + r * stride:off + r * stride + ln]
        pref.grad = gs[canon].clone()
        opt.step()
        gd = g.to(DEV)
        fold = dict(fold_off=b_off, fold_len=b_stride, fold_nrep=b_nrep, fold_stride=b_stride,
                    fold2_off=a_off, fold2_len=a_len, fold2_nrep=a_nrep, fold2_stride=a_stride)
        if opt_kind == "adam":
            K.adam_flat(p, gd, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, 1.0, step, arrive, 1, **fold)
        else:
            K.sgd_flat(p, gd, m, 1e-2, 0.9, 0.0, 0.0, False, 1.0, step, arrive, 1, **fold)
        torch.cuda.synchronize()
        _close(gd.cpu()[canon], gs[canon], 1e-6, 1e-6, f"folded grad step {it}")
        _close(gd.cpu()[~canon], g[~canon], 0, 0, f"replica storage step {it}")
    assert int(step.item()) == 4
    _close(p.cpu()[canon], pref.detach(), 0, 3e-6, f"{opt_kind} params")
    _close(p.cpu()[~canon], p0[~canon], 0, 0, "replica params untouched")


def test_engine_multi_step_tracks_torch_adam():
    B = 64
    net = build_net(seed=4, device=DEV)
    ref = torch_twin(net, dtype=torch.float32, device=DEV)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    n = 6 * B
    x, y = _batch(n, seed=9)
    xd, yd = x.to(DEV), y.to(DEV)
    eng = LeNetTrainStep(net, batch_size=B)
    eng.bind_dataset(xd, yd)
    eng.set_epoch_indices(torch.arange(n, dtype=torch.int32))
    for s in range(6):
        eng.step(B)
        sl = slice(s * B, (s + 1) * B)
        opt.zero_grad()
        torch.nn.functional.cross_entropy(ref(xd[sl]), yd[sl]).backward()
        opt.step()
    torch.cuda.synchronize()
    for (nm, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        _mostly_close(p, q, 2e-6, 6 * 2e-3, f"param after 6 steps {nm}")


def test_graph_replay_equals_eager():
    B = 128
    x, y = _batch(5 * B, seed=11)
    outs = []
    for use_graph in (False, True):
        net = build_net(seed=5, device=DEV)
        eng = LeNetTrainStep(net, batch_size=B)
        eng.bind_dataset(x.to(DEV), y.to(DEV))
        eng.set_epoch_indices(torch.arange(5 * B, dtype=torch.int32))
        eng.run_epoch(use_graph=use_graph)
        torch.cuda.synchronize()
        outs.append((eng.params.clone(), eng.read_meters()))
    assert int(outs[0][1][1]) == int(outs[1][1][1])
    _mostly_close(outs[1][0], outs[0][0], 2e-6, 5 * 2e-3, "graph vs eager params")


@pytest.mark.parametrize("B", [1, 37, 128])
def test_conv_fwd2_matches_v1_and_torch(B):
    """lenet_v2.hip conv forward (prefetched batch, LDS-DMA weights, 16x16x4 conv2 tiles) against the
    first-generation kernel and against the fp64 torch conv/pool chain."""
    from pytorch_distributed_example_amd._ext import kernels
    from pytorch_distributed_example_amd.ops.lenet_fused import LeNetWorkspace, pack_conv2_weight
    K = kernels()
    net = build_net(seed=6, device=DEV)
    x, _ = _batch(B, seed=40 + B)
    xd = x.to(DEV).reshape(B, 784).contiguous()
    w1, b1 = net.conv1.weight.detach().contiguous(), net.conv1.bias.detach().contiguous()
    w2, b2 = net.conv2.weight.detach().contiguous(), net.conv2.bias.detach().contiguous()
    ws1, ws2 = LeNetWorkspace(B, DEV), LeNetWorkspace(B, DEV)
    Wt2 = pack_conv2_weight(w2)
    K.lenet_conv_fwd(xd, None, None, 0, 0, None, B, w1, b1, Wt2, b2, ws1.P1, ws1.A1, ws1.P2, ws1.A2, None, None,
                     None)
    Wp = torch.zeros(2 * 72 * 256, device=DEV)
    K.lenet_pack_w2_v2(w2, Wp)
    K.lenet_conv_fwd2(xd, B, w1, b1, Wp, b2, ws2.P1, ws2.A1, ws2.P2, ws2.A2)
    torch.cuda.synchronize()
    xr = x.double()
    c1 = torch.nn.functional.conv2d(xr, w1.double().cpu(), b1.double().cpu()).relu()
    p1, i1 = torch.nn.functional.max_pool2d(c1, 2, 2, return_indices=True)
    c2 = torch.nn.functional.conv2d(p1, w2.double().cpu(), b2.double().cpu()).relu()
    p2 = torch.nn.functional.max_pool2d(c2, 2, 2)
    _close(ws2.P1.view(B, 20, 12, 12), p1, 1e-5, 1e-6, "P1 v2 vs torch")
    _close(ws2.P2.view(B, 50, 4, 4), p2, 1e-5, 1e-6, "P2 v2 vs torch")
    _close(ws2.P2, ws1.P2, 1e-5, 1e-6, "P2 v2 vs v1")
    _close(ws2.P1, ws1.P1, 1e-6, 1e-7, "P1 v2 vs v1")
    assert (ws2.A1 == ws1.A1).double().mean().item() > 0.999
    agree = (ws2.A2 == ws1.A2).double().mean().item()
    assert agree > 0.995, f"A2 argmax codes agree on only {agree:.4f}"     # ties broken by rounding order


def test_engine_v2_tracks_v1():
    """The v2 step (prefetch + new conv forward) trains like the first-generation step."""
    B, n = 128, 6 * 128
    x, y = _batch(n, seed=21)
    res = []
    for v2 in (False, True):
        net = build_net(seed=8, device=DEV)
        eng = LeNetTrainStep(net, batch_size=B, v2=v2)
        eng.bind_dataset(x.to(DEV), y.to(DEV))
        eng.set_epoch_indices(torch.randperm(n, generator=torch.Generator().manual_seed(2)).to(torch.int32))
        for _ in range(3):
            eng.step()
        eng.replay(steps=2)
        eng.replay(steps=1)
        torch.cuda.synchronize()
        res.append((torch.cat([p.detach().reshape(-1) for p in net.parameters()]), eng.read_meters()))
    _mostly_close(res[1][0], res[0][0], 2e-6, 6 * 2e-3, "v2 vs v1 params after 6 steps")
    assert abs(res[1][1][0] - res[0][1][0]) <= 1e-3 * abs(res[0][1][0]) + 1e-3


@pytest.mark.parametrize("mode", ["fold", "ext"])
def test_engine_v2_bit_reproducible(monkeypatch, mode):
    """Verdict r2 item 6: both comm-path reductions reduce the conv weight gradients in a fixed
    order -- "fold" (in-launch): conv2 slabs summed in group order by the last-arriving block, conv1
    as int64 fixed-point sums; "ext" (round 4 default): slabs and per-image conv1 partials stored
    plainly, summed in fixed order by k_conv_grad_fold -- so two identical runs give bit-identical
    parameters, gradients and moments.  (The W = 1 default "defer" keeps conv1's float atomics into
    16 replicas: fastest, reproducible to rounding only.)"""
    monkeypatch.setenv("PDE_LENET_BWD_MODE", mode)
    B, n = 128, 8 * 128
    x, y = _batch(n, seed=31)
    res = []
    for _ in range(2):
        net = build_net(seed=12, device=DEV)
        eng = LeNetTrainStep(net, batch_size=B)
        assert eng.bwd_mode == mode
        eng.bind_dataset(x.to(DEV), y.to(DEV))
        eng.set_epoch_indices(torch.randperm(n, generator=torch.Generator().manual_seed(5)).to(torch.int32))
        for _ in range(3):
            eng.step()
        eng.replay(steps=4)
        eng.replay(steps=1)
        torch.cuda.synchronize()
        res.append((eng.params.clone(), eng.grads.clone(), eng.m.clone(), eng.v.clone()))
    for a, b, what in zip(res[0], res[1], ("params", "grads", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), f"{what} differ between identical runs: {(a != b).sum().item()} elements"


def test_engine_bwd_modes_agree(monkeypatch):
    """The two places the conv gradients are reduced give the same training."""
    B, n = 128, 6 * 128
    x, y = _batch(n, seed=33)
    res = []
    for mode in ("defer", "fold", "ext"):
        monkeypatch.setenv("PDE_LENET_BWD_MODE", mode)
        net = build_net(seed=13, device=DEV)
        eng = LeNetTrainStep(net, batch_size=B)
        eng.bind_dataset(x.to(DEV), y.to(DEV))
        eng.set_epoch_indices(torch.arange(n, dtype=torch.int32))
        for _ in range(6):
            eng.step()
        torch.cuda.synchronize()
        res.append(torch.cat([p.detach().reshape(-1) for p in net.parameters()]))   # layouts differ by mode
    _mostly_close(res[1], res[0], 1e-7, 2e-5, "fold vs defer")
    _mostly_close(res[2], res[0], 1e-7, 2e-5, "ext vs defer")


@pytest.mark.parametrize("mode", ["fold", "ext"])
def test_engine_comm_modes_propagate_nonfinite(monkeypatch, mode):
    """a non-finite gradient must stay non-finite through the comm-path reductions (the
    int64 fixed-point conv1 fold used to turn NaN into a finite garbage value)."""
    monkeypatch.setenv("PDE_LENET_BWD_MODE", mode)
    B, n = 128, 2 * 128
    x, y = _batch(n, seed=35)
    net = build_net(seed=14, device=DEV)
    with torch.no_grad():
        net.fc2.bias[0] = float("nan")      # logits -> dlogits -> every backward operand
    eng = LeNetTrainStep(net, batch_size=B)
    eng.bind_dataset(x.to(DEV), y.to(DEV))
    eng.set_epoch_indices(torch.arange(n, dtype=torch.int32))
    eng.step()
    torch.cuda.synchronize()
    for name in ("conv1.weight", "conv1.bias", "conv2.weight"):
        assert not bool(torch.isfinite(eng.g[name]).all()), f"{name}: NaN input gave a finite gradient"


def test_engine_rejects_unknown_bwd_mode(monkeypatch):
    monkeypatch.setenv("PDE_LENET_BWD_MODE", "v1")
    with pytest.raises(ValueError):
        LeNetTrainStep(build_net(seed=1, device=DEV), batch_size=128)



def test_bench_plain_run_dumps_reproducible_step_outputs(tmp_path, capsys, monkeypatch):
    """``bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR``: a plain run prints one result line
    for the K timed steps without the ``--full`` figures, then writes what one step of the timed path
    computes from the seeded start state (updated parameters, per-row loss / hit flags, meters) as
    float32 / float64 .npy files -- the same from run to run, whatever K and W were.
    (``bench.main`` in this process: no second interpreter start; the host-thread pinning and wait
    policy it would set for a process of its own stay off.)

    Bound between two runs: everything but the conv1 gradient sums (float atomics) is computed in a
    fixed order, and Adam's first update lr * g / (|g| + eps) moves with a rounding difference d in g
    by lr * eps * d / (|g| + eps)^2 -- below 1e-9 unless |g| is itself within rounding of zero, where
    it can reach the whole step.  So at least 99 % of every array agree within 1e-6 (float32
    resolution of parameters below 1) and no element differs by more than 2 * lr; the losses come
    from the forward pass of the identical start state and agree to float32 rounding."""
    import json
    import os

    import numpy as np

    import bench
    monkeypatch.setenv("PDE_BENCH_NUMA", "0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PDE_BENCH_STUB", "PDE_BENCH_RESULT"):
        monkeypatch.delenv(k, raising=False)
    shapes = {"param." + n: tuple(q.shape) for n, q in build_net(seed=0, device="cpu").named_parameters()}
    shapes.update(row_loss=(128,), row_hit=(128,), loss_sum=(1,), correct=(1,))
    runs = []
    for name, steps, warmup in (("a", "4", "2"), ("b", "7", "3")):
        out = tmp_path / name
        capsys.readouterr()
        bench.main(["--gpus", "1", "--steps", steps, "--warmup", warmup, "--train-size", "2048", "--no-spin-wait",
                    "--dump-outputs", str(out)])
        lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        assert d["steps"] == int(steps) and d["ms_per_step"] > 0 and d["dtype"] == "fp32" and "w1_rccl_comm" not in d
        assert abs(d["value"] - 128 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
        assert 0 < d["train_loss_mean_timed_rank0"] < 10           # the line's meters are the timed steps'
        assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in shapes)
        got = {k: np.load(out / (k + ".npy")) for k in shapes}
        for k, a in got.items():
            assert a.shape == shapes[k] and np.isfinite(a).all(), k
            assert a.dtype == (np.float64 if k in ("loss_sum", "correct", "row_hit") else np.float32), k
        assert sum(a.nbytes for a in got.values()) <= 64 << 20
        assert set(np.unique(got["row_hit"])) <= {0.0, 1.0} and (got["row_loss"] >= 0).all()
        # the dumped meters are those of the one output step of 128 rows
        assert abs(got["loss_sum"][0] - got["row_loss"].astype(np.float64).sum()) <= 1e-3
        assert got["correct"][0] == got["row_hit"].sum()
        runs.append(got)
    # the step really trained: the parameters left the seeded initial values by about lr
    init = dict(build_net(seed=0, device="cpu").named_parameters())
    moved = np.abs(runs[0]["param.fc1.weight"] - init["fc1.weight"].detach().numpy())
    assert 1e-4 < moved.mean() <= 1.01e-3
    for k in shapes:
        diff = np.abs(runs[0][k].astype(np.float64) - runs[1][k].astype(np.float64)).reshape(-1)
        print(f"{k}: max diff {diff.max():.3e}, above 1e-6: {(diff > 1e-6).sum()} of {diff.size}")
        if k.startswith("param."):
            assert (diff <= 1e-6).mean() >= 0.99 and diff.max() <= 2e-3, k
        elif k == "loss_sum":
            assert diff.max() <= 1e-3, k             # 128 float32 losses of order 1, summed in float64
        elif k == "row_loss":
            assert diff.max() <= 1e-5, k
        else:
            assert diff.max() == 0, k
