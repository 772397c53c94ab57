"""Learning-rate tables on the GPU (optim.lr_scheduler): the optimizer kernels read the rate of step t
from a device table with their device step count, so a captured step follows a schedule on replay.

Wherever a comparison is bit-identical, its other arm is the by-value path fed the same fp32 rate
from the host for every step, so no tolerance is involved.  The table has a zero first rate
(parameters unchanged, moments updated), changes on every step, and the runs go 3 steps past its end.
"""
import os
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd._ext import kernels
from pytorch_distributed_example_amd.engine import LeNetTrainStep
from pytorch_distributed_example_amd.models import build_net
from pytorch_distributed_example_amd.optim import SGD, Adam, AdamW, AdamWMaster, LRTable, SGDMaster
from pytorch_distributed_example_amd.utils.checkpoint import load_checkpoint, save_checkpoint

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))

LRS = [0.0, 5e-4, 1e-3, 7.5e-4, 2.5e-4]
STEPS = 8


def _table(lrs=LRS, device=dev):
    return torch.tensor(lrs, dtype=torch.float64).to(torch.float32).to(device)


def _lr_at(k, lrs=LRS):
    return float(_table(lrs, "cpu")[min(k, len(lrs) - 1)])


FUSED = [(Adam, torch.optim.Adam, {}), (AdamW, torch.optim.AdamW, dict(weight_decay=1e-2)),
         (SGD, torch.optim.SGD, dict(momentum=0.9))]


def _fused_state(opt):
    fg = opt._flat[0]
    return [fg.params] + list(fg.bufs.values()) + [fg.step_ctr]


# ---------------------------------------------------------------- 1. eager, fused fp32 optimizers
@pytest.mark.parametrize("opt_cls,ref_cls,kw", FUSED)
def test_fused_eager_table_is_host_lr_bit_for_bit(opt_cls, ref_cls, kw):
    nets = [build_net(seed=1, device=dev) for _ in range(3)]
    oa = opt_cls(nets[0].parameters(), lr=123.0, **kw)           # 123.0: the kernel must ignore it
    oa.set_lr_table(_table())
    ob = opt_cls(nets[1].parameters(), lr=1e-3, **kw)
    oc = ref_cls(nets[2].parameters(), lr=1.0, foreach=False, **kw)
    sc = torch.optim.lr_scheduler.LambdaLR(oc, lambda k: _lr_at(k))
    torch.manual_seed(0)
    p_start = oa.param_groups[0]["params"][0].detach().clone()
    for k in range(STEPS):
        x = torch.randn(8, 1, 28, 28, device=dev)
        y = torch.randint(0, 10, (8,), device=dev)
        ob.param_groups[0]["lr"] = _lr_at(k)
        for net, opt in zip(nets, (oa, ob, oc)):
            opt.zero_grad()
            F.cross_entropy(net(x), y).backward()
            opt.step()
        sc.step()
        assert oa.param_groups[0]["lr"] == 123.0
        for a, b in zip(_fused_state(oa), _fused_state(ob)):
            assert torch.equal(a, b), f"step {k + 1}: {(a != b).sum().item()} elements differ"
        if k == 0:      # rate 0: parameters unchanged, the moments moved
            assert torch.equal(oa.param_groups[0]["params"][0], p_start)
            assert all(bool(b.abs().sum() > 0) for b in oa._flat[0].bufs.values())
    assert not torch.equal(oa.param_groups[0]["params"][0], p_start)
    assert oa.lr_step_count() == STEPS
    for p, q in zip(nets[0].parameters(), nets[2].parameters()):
        d = (p - q).abs()
        assert d.mean().item() < 1e-5 and d.max().item() < 5e-4


# ---------------------------------------------------------------- 2. graph replay, master optimizers
SHAPES = [(64,), (5, 37), (129, 64), (3, 3, 7)]
MASTER = [(AdamWMaster, dict(lr=1e-3, max_grad_norm=1.0)), (SGDMaster, dict(lr=1e-3, momentum=0.9))]


def _bf16_params(seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).to(dev, torch.bfloat16).requires_grad_() for s in SHAPES]


def _master_setup(opt_cls, kw, capturable, table=None):
    """The optimizer built and its gradients bound to the flat buffer (so a captured step copies nothing)."""
    ps = _bf16_params()
    opt = opt_cls(ps, capturable=capturable, **kw)
    if table is not None:
        opt.set_lr_table(table)
    opt.state_tensors()
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt._sync_grads()
    return ps, opt


def _master_grads(ps, opt, n=STEPS):
    """n fixed flat gradient buffers (padding between parameters stays zero)."""
    g = torch.Generator().manual_seed(12)
    out = []
    for _ in range(n):
        for p in ps:
            p.grad.copy_(torch.randn(*p.shape, generator=g).to(dev))
        out.append(opt._flat["g"].clone())
    return out


def _master_state(opt):
    f = opt._flat
    return [f["p"]] + list(f["bufs"].values())


def _eager_host_lr(opt_cls, kw, G, lrs=LRS, steps=STEPS):
    ps, opt = _master_setup(opt_cls, kw, capturable=False)
    for k in range(steps):
        for g in opt.param_groups:
            g["lr"] = _lr_at(k, lrs)
        opt._flat["g"].copy_(G[k])
        opt.step()
    torch.cuda.synchronize()
    return opt


def _replay(opt_cls, kw, G, table):
    ps, opt = _master_setup(opt_cls, kw, capturable=True, table=table)
    opt._flat["g"].copy_(G[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k in range(STEPS):
        opt._flat["g"].copy_(G[k])
        graph.replay()
    torch.cuda.synchronize()
    return opt


@pytest.mark.parametrize("opt_cls,kw", MASTER)
def test_master_graph_replay_follows_table(opt_cls, kw):
    ps, o0 = _master_setup(opt_cls, kw, capturable=False)
    G = _master_grads(ps, o0)
    ref = _eager_host_lr(opt_cls, kw, G)
    got = _replay(opt_cls, kw, G, _table())
    frozen = _replay(opt_cls, kw, G, None)          # no table: the captured by-value rate, every replay
    assert got.lr_step_count() == STEPS and frozen.lr_step_count() == STEPS
    names = ["bf16 weights"] + list(ref._flat["bufs"])
    for a, b, what in zip(_master_state(got), _master_state(ref), names):
        assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} elements differ from the host-lr loop"
    assert not torch.equal(ref._flat["bufs"]["master"], o0._flat["bufs"]["master"])    # it trained
    # the run without a table finished cleanly above; it cannot have followed the schedule
    assert not torch.equal(frozen._flat["bufs"]["master"], ref._flat["bufs"]["master"])
    assert not torch.equal(frozen._flat["p"], ref._flat["p"])


# ---------------------------------------------------------------- 3. toy-CNN engine
def _epoch(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 1, 28, 28, generator=g).to(dev), torch.randint(0, 10, (n,), generator=g).to(dev)


ENGINE = [("adam", dict(lr=1e-3)), ("sgd", dict(lr=1e-3, momentum=0.9))]


def _engine(opt, kw, x, y, idx=None, seed=5, B=16, **extra):
    net = build_net(seed=seed, device=dev)
    eng = LeNetTrainStep(net, batch_size=B, optimizer=opt, **kw, **extra)
    eng.bind_dataset(x, y)
    eng.set_epoch_indices(torch.arange(x.shape[0], dtype=torch.int32) if idx is None else idx)
    return eng


def _engine_state(eng):
    return [eng.params, eng.m, eng.v, eng.counters]


@pytest.mark.parametrize("opt,kw", ENGINE)
def test_engine_multi_step_replay_follows_table(opt, kw):
    """B=16: one image per conv1 gradient replica, so the default W=1 step is order-free."""
    x, y = _epoch(STEPS * 16, 41)
    a = _engine(opt, kw, x, y, lr_schedule=LRS)
    p0 = a.params.clone()
    for s in (3, 3, 2):
        a.replay(steps=s)
    b = _engine(opt, kw, x, y)
    for k in range(STEPS):
        b.lr = _lr_at(k)
        b.graphs.clear()
        b.replay(steps=1)
    torch.cuda.synchronize()
    for s, t, what in zip(_engine_state(a), _engine_state(b), ("params", "m", "v", "counters")):
        assert torch.equal(s, t), f"{what}: {(s != t).sum().item()} elements differ"
    assert int(a.counters[0]) == STEPS and not torch.equal(a.params, p0)
    assert a.current_lr() == _lr_at(STEPS)
    assert a.optimizer_state_dict()["param_groups"][0]["lr"] == _lr_at(STEPS)
    sched = LRTable(b, LRS)                           # attaches to an engine that already ran 8 steps
    assert sched.get_last_lr() == [_lr_at(STEPS)] and sched.last_epoch == STEPS


def _run_lr_worker(case, world, *args, extra_env=None):
    from pytorch_distributed_example_amd.launch import free_port, run_gang
    sys.path.insert(0, HERE)
    import json
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, os.path.join(HERE, "mp_lr_workers.py"), case, *map(str, args)]
        env = {"PYTHONWARNINGS": "ignore::FutureWarning"}
        env.update(extra_env or {})
        rc = run_gang(cmd, world, "127.0.0.1", free_port(), log_dir=d, extra_env=env)
        logs = [open(os.path.join(d, f"rank{r}.log")).read() for r in range(world)]
    res = []
    for log in logs:
        rows = [json.loads(l[len("RESULT "):]) for l in log.splitlines() if l.startswith("RESULT ")]
        res.append(rows[-1] if rows else None)
    return rc, res, logs


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_engine_ext_mode_comm_path_follows_table(opt):
    """PDE_LENET_BWD_MODE=ext in a child process with the comm path forced on (one rank): the ext-mode
    gradient fold and the separate fc / conv optimizer launches both read the same counters[0]."""
    rc, res, logs = _run_lr_worker("engine_ext", 1, opt, extra_env={"PDE_LENET_BWD_MODE": "ext"})
    assert rc == 0, "\n".join(logs)
    assert res[0]["same"] == [True, True, True, True], res[0]
    assert res[0]["steps"] == STEPS


# ---------------------------------------------------------------- 4. a table of length 1
@pytest.mark.parametrize("opt_cls,ref_cls,kw", FUSED)
def test_fused_length_one_table_is_no_table(opt_cls, ref_cls, kw):
    nets = [build_net(seed=2, device=dev) for _ in range(2)]
    oa = opt_cls(nets[0].parameters(), lr=1e-3, **kw)
    oa.set_lr_table(_table([1e-3]))
    ob = opt_cls(nets[1].parameters(), lr=1e-3, **kw)
    torch.manual_seed(3)
    for _ in range(3):
        x = torch.randn(8, 1, 28, 28, device=dev)
        y = torch.randint(0, 10, (8,), device=dev)
        for net, opt in zip(nets, (oa, ob)):
            opt.zero_grad()
            F.cross_entropy(net(x), y).backward()
            opt.step()
    for a, b in zip(_fused_state(oa), _fused_state(ob)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("opt_cls,kw", MASTER)
def test_master_length_one_table_is_no_table(opt_cls, kw):
    ps, o0 = _master_setup(opt_cls, kw, capturable=False)
    G = _master_grads(ps, o0, 3)
    res = []
    for table in (_table([kw["lr"]]), None):
        _, opt = _master_setup(opt_cls, kw, capturable=False, table=table)
        for k in range(3):
            opt._flat["g"].copy_(G[k])
            opt.step()
        res.append(opt)
    for a, b in zip(_master_state(res[0]), _master_state(res[1])):
        assert torch.equal(a, b)
    assert not torch.equal(res[0]._flat["bufs"]["master"], o0._flat["bufs"]["master"])


@pytest.mark.parametrize("opt,kw", ENGINE)
def test_engine_length_one_table_is_no_table(opt, kw):
    x, y = _epoch(3 * 16, 43)
    a = _engine(opt, kw, x, y, lr_schedule=[kw["lr"]])
    b = _engine(opt, kw, x, y)
    a.replay(steps=3)
    b.replay(steps=3)
    torch.cuda.synchronize()
    for s, t in zip(_engine_state(a), _engine_state(b)):
        assert torch.equal(s, t)


# ---------------------------------------------------------------- 5. resume
def test_engine_resume_continues_schedule(tmp_path):
    x, y = _epoch(STEPS * 16, 45)
    kw = dict(lr=1e-3)
    full = _engine("adam", kw, x, y)
    LRTable(full, LRS)
    for _ in range(STEPS):
        full.step()
    first = _engine("adam", kw, x, y)
    s1 = LRTable(first, LRS)
    for _ in range(4):
        first.step()
    s1.step(4)
    ck = str(tmp_path / "ck.pt")
    save_checkpoint(ck, first.net, first.optimizer_state_dict(), epoch=1, extra={"lr_scheduler": s1.state_dict()})
    # a fresh engine and scheduler; the epoch's remaining four batches
    second = _engine("adam", kw, x, y, idx=torch.arange(4 * 16, STEPS * 16, dtype=torch.int32), seed=99)
    s2 = LRTable(second, [9.0])
    payload = load_checkpoint(ck, second.net)
    second.load_optimizer_state_dict(payload["optimizer"])
    s2.load_state_dict(payload["extra"]["lr_scheduler"])
    assert s2.last_epoch == 4 and s2.get_last_lr() == [_lr_at(4)]
    assert payload["optimizer"]["param_groups"][0]["lr"] == _lr_at(4)
    for _ in range(4):
        second.step()
    torch.cuda.synchronize()
    for n in full.layout.param_names:
        for buf_a, buf_b, what in ((full.params, second.params, "param"), (full.m, second.m, "m"),
                                   (full.v, second.v, "v")):
            assert torch.equal(full.layout.view(buf_a, n), second.layout.view(buf_b, n)), f"{what} {n}"
    assert int(second.counters[0]) == STEPS == int(full.counters[0])


# ---------------------------------------------------------------- 6. shared-GPU DDP
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_engine_ddp_w2_follows_table(opt):
    """Two ranks sharing the GPU, 6 steps under the table: bit-identical replicas that equal one rank
    on the concatenated shards within the bounds of test_engine_w2_matches_w1_on_concatenated_shards."""
    rc, res, logs = _run_lr_worker("engine_ddp", 2, "6", opt, extra_env={"PDE_PEER_TIMEOUT_MS": "120000"})
    assert rc == 0, "\n".join(logs)
    assert res[0]["bits"] == res[1]["bits"], "replicas diverged"
    lrs = [50 * x for x in LRS] if opt == "sgd" else LRS          # as the worker scales them
    assert res[0]["steps"] == res[1]["steps"] == 6
    assert res[0]["lr_next"] == res[1]["lr_next"] == _lr_at(6, lrs)
    r = res[0]
    w, one = r["w_loss"], r["one_loss"]
    assert len(w) == len(one) == 6
    for a, b in zip(w, one):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (w, one)
    if opt == "sgd":
        for d, up, pm in zip(r["max_abs_diff"], r["max_update"], r["max_param"]):
            assert d <= 1e-5 * pm, (r["max_abs_diff"], r["max_param"])
            assert up > 1e-3 * pm
    else:
        for a, b in zip(r["w_params"], r["one_params"]):
            assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (r["w_params"], r["one_params"])
    # the run with the constructor's rate frozen is a different training
    assert any(abs(a - b) > 1e-4 * max(1.0, abs(b)) for a, b in zip(r["frozen_params"], r["one_params"]))


# ---------------------------------------------------------------- 7. host validation
def test_bad_tables_raise_before_any_launch():
    K = kernels()
    n = 1024
    p = torch.ones(n, device=dev)
    g, m, v = torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, device=dev, dtype=torch.int64)
    arrive = torch.zeros(1, device=dev, dtype=torch.int32)
    bad = {"CPU": (_table(device="cpu"), "is on cpu"), "float64": (_table().double(), "float32"),
           "empty": (torch.zeros(0, device=dev), "empty")}
    for what, (tab, msg) in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            K.adam_flat(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, 1.0, step, arrive, 1, lr_table=tab)
        with pytest.raises(RuntimeError, match=msg):
            K.sgd_flat(p, g, m, 1e-3, 0.9, 0.0, 0.0, False, 1.0, step, arrive, 1, lr_table=tab)
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and int(step) == 0 and not bool(m.any())           # nothing was launched
    p16 = torch.ones(n, device=dev, dtype=torch.bfloat16)
    for what, (tab, msg) in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            K.adamw_master(p, p16, p16, m, v, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1.0, 1, lr_table=tab)
        with pytest.raises(RuntimeError, match=msg):
            K.sgd_master(p, p16, p16, m, 1e-3, 0.9, 0.0, False, 1.0, None, lr_table=tab)
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and bool((p16 == 1).all())
    # the optimizers and the engine refuse the same tables when they are attached
    net = build_net(seed=1, device=dev)
    ps = list(net.parameters())
    for opt in (Adam([{"params": ps[:2]}, {"params": ps[2:]}], lr=1e-3), AdamWMaster(_bf16_params()),
                SGDMaster(_bf16_params())):
        ng = len(opt.param_groups)
        with pytest.raises(ValueError, match="is on cpu"):
            opt.set_lr_table(_table(device="cpu"))
        with pytest.raises(TypeError, match="float32"):
            opt.set_lr_table(_table().double())
        with pytest.raises(ValueError, match="at least one rate"):
            opt.set_lr_table(torch.zeros(0, device=dev))
        with pytest.raises(ValueError, match=f"{ng + 1} learning-rate tables for {ng} parameter groups"):
            opt.set_lr_table([_table()] * (ng + 1))
        with pytest.raises(ValueError, match="parameter groups"):
            LRTable(opt, [LRS] * (ng + 1))
    eng = LeNetTrainStep(net, batch_size=16)
    with pytest.raises(ValueError, match="is on cpu"):
        eng.set_lr_table(_table(device="cpu"))
    with pytest.raises(TypeError, match="float32"):
        eng.set_lr_table(_table().double())
    with pytest.raises(ValueError, match="at least one rate"):
        eng.set_lr_table([])
