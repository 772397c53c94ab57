"""Learning-rate tables (optim.lr_scheduler) without a GPU: parity of the tables with
torch.optim.lr_scheduler, the scheduler surface, the CPU optimizer paths under a table, and the
--lr-schedule flags of scripts/mnist.py on the CPU/gloo path."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd.models import MLP
from pytorch_distributed_example_amd.optim import SGD, Adam, LRTable, lr_scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONWARNINGS="ignore::FutureWarning", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
STEPS = 50


def _f32(xs):
    return torch.tensor([float(x) for x in xs], dtype=torch.float64).to(torch.float32)


def _warmup_cosine_lambda(k, warmup=5, total=STEPS):
    if k < warmup:
        return (k + 1) / warmup
    return 0.5 * (1.0 + math.cos(math.pi * (k - warmup) / (total - warmup)))


FACTORIES = {
    "lambda": lambda o: torch.optim.lr_scheduler.LambdaLR(o, _warmup_cosine_lambda),
    "steplr": lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=7, gamma=0.5),
    "onecycle": lambda o: torch.optim.lr_scheduler.OneCycleLR(o, max_lr=1e-2, total_steps=STEPS),
}


def _torch_lrs(factory, base_lr, steps):
    """The learning rate torch uses for optimizer step k+1, k = 0..steps-1."""
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=base_lr)
    sched = factory(opt)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("name", sorted(FACTORIES))
def test_from_torch_table_equals_torch(name):
    net = MLP()
    opt = Adam(net.parameters(), lr=3e-3)
    sched = lr_scheduler.from_torch(opt, FACTORIES[name], STEPS)
    want = _f32(_torch_lrs(FACTORIES[name], 3e-3, STEPS))
    assert sched.tables[0].dtype == torch.float32 and sched.tables[0].shape == (STEPS,)
    assert torch.equal(sched.tables[0], want)
    assert len(set(want.tolist())) > 3                     # a schedule that really moves


def test_warmup_cosine_formula():
    base, warm, total, lo = 2e-3, 4, 20, 1e-5
    lrs = lr_scheduler.warmup_cosine(base, warm, total, lo)
    assert len(lrs) == total
    assert lrs[0] == base / warm                            # first entry base_lr / warmup_steps, not 0
    assert lrs[warm - 1] == base and max(lrs) == base       # the peak: the rate of optimizer step `warm`
    assert lrs[-1] == lo
    for k in range(total):
        want = (base * (k + 1) / warm if k < warm else
                lo + 0.5 * (base - lo) * (1.0 + math.cos(math.pi * (k + 1 - warm) / (total - warm))))
        assert lrs[k] == want
    assert all(a > b for a, b in zip(lrs[warm - 1:], lrs[warm:]))   # strictly decreasing after the peak
    assert lr_scheduler.constant(0.5) == [0.5]


def test_step_decay_equals_steplr():
    lrs = lr_scheduler.step_decay(1e-2, 7, 0.5, STEPS)
    assert torch.equal(_f32(lrs), _f32(_torch_lrs(FACTORIES["steplr"], 1e-2, STEPS)))
    assert lrs == _torch_lrs(FACTORIES["steplr"], 1e-2, STEPS)      # the doubles too


def test_scheduler_surface_and_state_round_trip():
    table = [0.0, 5e-4, 1e-3, 7.5e-4, 2.5e-4]
    f32 = _f32(table).tolist()
    net = MLP()
    opt = SGD(net.parameters(), lr=123.0)
    sched = LRTable(opt, table)
    assert sched.last_epoch == 0 and opt.param_groups[0]["lr"] == f32[0]
    for k in range(1, 9):
        sched.step()
        want = f32[min(k, len(f32) - 1)]
        assert sched.last_epoch == k
        assert sched.get_last_lr() == [want] and opt.param_groups[0]["lr"] == want
    sd = sched.state_dict()
    other = LRTable(SGD(MLP().parameters(), lr=1.0), [9.0, 8.0])
    other.load_state_dict(sd)
    assert other.last_epoch == 8 and other.get_last_lr() == [f32[-1]]
    assert torch.equal(other.tables[0], _f32(table))
    sd2 = other.state_dict()
    assert sd2["last_epoch"] == sd["last_epoch"] and all(torch.equal(a, b) for a, b in zip(sd2["tables"], sd["tables"]))
    # position only (what a resumed CLI run restores)
    third = LRTable(SGD(MLP().parameters(), lr=1.0), table)
    third.load_state_dict({"last_epoch": 3})
    assert third.get_last_lr() == [f32[3]]


def test_per_group_tables_and_validation():
    net = MLP()
    ps = list(net.parameters())
    opt = Adam([{"params": ps[:2]}, {"params": ps[2:]}], lr=1e-3)
    sched = LRTable(opt, [[1e-3, 2e-3], [5e-4]])
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [_f32([2e-3]).item(), _f32([5e-4]).item()]
    with pytest.raises(ValueError, match="3 learning-rate lists for 2 parameter groups"):
        LRTable(opt, [[1e-3], [1e-3], [1e-3]])
    with pytest.raises(ValueError, match="3 learning-rate tables for 2 parameter groups"):
        opt.set_lr_table([torch.ones(2)] * 3)
    with pytest.raises(TypeError, match="float32"):
        opt.set_lr_table(torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="at least one rate"):
        opt.set_lr_table(torch.ones(0))
    with pytest.raises(ValueError):
        LRTable(opt, [])
    opt.set_lr_table(None)


def _train_mlp(opt, sched, steps=10):
    torch.manual_seed(0)
    net = opt._net
    for _ in range(steps):
        x = torch.randn(8, 1, 28, 28)
        y = torch.randint(0, 10, (8,))
        opt.zero_grad()
        F.nll_loss(net(x), y).backward()
        opt.step()
        sched.step()
    return net


@pytest.mark.parametrize("opt_cls,ref_cls,kw", [
    (Adam, torch.optim.Adam, dict(lr=1e-3)),
    (SGD, torch.optim.SGD, dict(lr=1e-2, momentum=0.9)),
])
def test_cpu_optimizer_under_table_matches_torch(opt_cls, ref_cls, kw):
    """The CPU paths read group["lr"], which LRTable.step() writes: same tolerance as
    test_core_cpu.test_optimizer_cpu_matches_torch."""
    # cycle_momentum off: a table schedules the learning rate only (no momentum / beta schedules)
    factory = lambda o: torch.optim.lr_scheduler.OneCycleLR(o, max_lr=10 * kw["lr"], total_steps=10,
                                                            cycle_momentum=False)
    torch.manual_seed(1)
    a = MLP()
    b = MLP()
    b.load_state_dict(a.state_dict())
    oa, ob = opt_cls(a.parameters(), **kw), ref_cls(b.parameters(), **kw)
    oa._net, ob._net = a, b
    start = [p.detach().clone() for p in a.parameters()]
    sa = lr_scheduler.from_torch(oa, factory, 10)
    sb = factory(ob)
    _train_mlp(oa, sa)
    _train_mlp(ob, sb)
    moved = False
    for p, q, p0 in zip(a.parameters(), b.parameters(), start):
        assert torch.allclose(p, q, atol=1e-6, rtol=1e-5)
        moved = moved or not torch.equal(p, p0)
    assert moved


# ---------------------------------------------------------------------------------------------- CLI
def _mnist(args, n, timeout=300):
    base = [os.path.join(ROOT, "scripts/mnist.py"), "--no-cuda", "--backend", "gloo", "--train-size", "1024",
            "--test-size", "256", "--epochs", "2", "--no-cprofile", "--model", "mlp"] + args
    launch = ["-m", "pytorch_distributed_example_amd.launch", "-n", str(n)]
    out = subprocess.run([sys.executable] + launch + base, cwd=ROOT, capture_output=True, text=True, env=ENV,
                         timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


@pytest.mark.parametrize("world", [1, 2])
def test_cli_cosine_metrics_lr_follows_table(world, tmp_path):
    metrics = str(tmp_path / "m.jsonl")
    lines = _mnist(["--eval", "--lr-schedule", "cosine", "--lr-warmup", "3", "--lr-min", "1e-5", "--metrics", metrics],
                   world)
    per_epoch = math.ceil(1024 / world / 128)
    table = _f32(lr_scheduler.warmup_cosine(1e-3, 3, 2 * per_epoch, 1e-5)).tolist()
    recs = [json.loads(l) for l in open(metrics)]
    # each epoch's row carries the rate of the epoch's last optimizer step
    assert [r["lr"] for r in recs] == [table[per_epoch - 1], table[2 * per_epoch - 1]]
    assert recs[-1]["lr"] == _f32([1e-5]).item()
    ep = [l for l in lines if l.startswith("Epoch: ")]
    assert len(ep) == 2 * world
    for e in ("1", "2"):                                   # ranks print identical test metrics
        assert len({l.split("test loss:")[1] for l in ep if l.startswith(f"Epoch: {e}/")}) == 1
    # the schedule is in effect: a constant-rate run trains differently
    const = [l for l in _mnist(["--eval"], world) if l.startswith("Epoch: ")]
    assert const != ep


@pytest.mark.parametrize("world", [1, 2])
def test_cli_constant_is_byte_identical(world, tmp_path):
    m0, m1 = str(tmp_path / "a.jsonl"), str(tmp_path / "b.jsonl")
    strip = lambda ls: sorted(l for l in ls if not l.startswith("Namespace("))
    a = _mnist(["--eval", "--log-rank0-only", "--metrics", m0], world)
    b = _mnist(["--eval", "--log-rank0-only", "--lr-schedule", "constant", "--metrics", m1], world)
    ns = [l for l in a if l.startswith("Namespace(")]
    assert [l.replace(m1, m0) for l in b if l.startswith("Namespace(")] == ns     # same line: only the path differs
    assert strip(a) == strip(b)
    ra, rb = [json.loads(l) for l in open(m0)], [json.loads(l) for l in open(m1)]
    assert [r["line"] for r in ra] == [r["line"] for r in rb] and all("lr" not in r for r in ra + rb)
