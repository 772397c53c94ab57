"""Worker bodies of the learning-rate-table tests that need their own process (the pattern of
``mp_workers.py``: one process per rank under ``launch.run_gang``, ``RESULT <json>`` lines).

  engine_ext   one rank, PDE_LENET_BWD_MODE=ext set by the parent, the comm path forced on: the
               ext-mode gradient fold and the separate fc / conv optimizer launches of the "overlap"
               schedule, a scheduled engine against a by-value one
  engine_ddp   W ranks sharing cuda:0 (peer all-reduce), toy-CNN DDP under a table, against one rank
               on the concatenated shards
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mp_workers import R, W, _dev, _init, _shared_gpu_init, emit  # noqa: E402
from pytorch_distributed_example_amd import dist  # noqa: E402

LRS = [0.0, 5e-4, 1e-3, 7.5e-4, 2.5e-4]


def _table():
    return torch.tensor(LRS, dtype=torch.float64).to(torch.float32)


def _bits(t):
    return int(t.detach().contiguous().view(torch.int32).to(torch.int64).sum().item())


def case_engine_ext(opt="adam"):
    from pytorch_distributed_example_amd.engine import LeNetTrainStep
    from pytorch_distributed_example_amd.models import build_net

    assert os.environ.get("PDE_LENET_BWD_MODE") == "ext"
    _init("nccl")
    dev = _dev("nccl")
    B, n = 16, 8 * 16
    g = torch.Generator().manual_seed(41)
    x, y = torch.randn(n, 1, 28, 28, generator=g).to(dev), torch.randint(0, 10, (n,), generator=g).to(dev)
    kw = dict(optimizer="sgd", lr=1e-3, momentum=0.9) if opt == "sgd" else dict(lr=1e-3)
    tab = _table()
    out = []
    for scheduled in (True, False):
        net = build_net(seed=5, device=dev)
        eng = LeNetTrainStep(net, batch_size=B, comm=dist.engine_comm(), force_comm=True,
                             lr_schedule=LRS if scheduled else None, **kw)
        assert eng.bwd_mode == "ext" and eng.comm_on and eng.mode == "overlap"
        eng.bind_dataset(x, y)
        eng.set_epoch_indices(torch.arange(n, dtype=torch.int32))
        if scheduled:
            for s in (3, 3, 2):
                eng.replay(steps=s)
        else:
            for k in range(8):
                eng.lr = float(tab[min(k, len(LRS) - 1)])
                eng.graphs.clear()
                eng.replay(steps=1)
        torch.cuda.synchronize()
        out.append([eng.params.clone(), eng.m.clone(), eng.v.clone(), eng.counters.clone()])
    same = [bool(torch.equal(a, b)) for a, b in zip(*out)]
    emit({"same": same, "steps": int(out[0][3][0].item()), "bits": _bits(out[0][0])})
    dist.destroy_process_group()


def case_engine_ddp(steps="6", opt="adam"):
    from pytorch_distributed_example_amd.data import DistributedSampler, synthetic_mnist
    from pytorch_distributed_example_amd.engine import LeNetTrainStep
    from pytorch_distributed_example_amd.models import build_net

    n_steps, b = int(steps), 64
    # sgd: the table scaled by 50 (peak 0.05, the rate of mp_workers.case_engine_w2_equiv), so the
    # parameters move by far more than the comparison's bound
    kw = dict(optimizer="sgd", lr=0.05, momentum=0.9) if opt == "sgd" else {}
    lrs = [50 * x for x in LRS] if opt == "sgd" else LRS
    dev = _shared_gpu_init()
    ds = synthetic_mnist(2048, seed=0, device=dev)
    shards = [DistributedSampler(ds, num_replicas=W, rank=r, shuffle=True, seed=0).indices_tensor()
              for r in range(W)]

    def train(eng, idx):
        eng.bind_dataset(ds.images, ds.labels)
        eng.set_epoch_indices(idx)
        out = []
        for _ in range(n_steps):
            eng.step()
            loss, _, _ = eng.read_meters()
            out.append(loss)
        return out

    net = build_net(seed=3, device=dev)
    net0 = [p.detach().clone() for p in net.parameters()]
    comm = dist.engine_comm(allow_host_only=True)
    eng = LeNetTrainStep(net, batch_size=b, comm=comm, force_comm=True, lr_schedule=lrs, **kw)
    mine = train(eng, shards[R])
    torch.cuda.synchronize()
    assert comm.health() == "", comm.health()
    tot = torch.tensor(mine, dtype=torch.float64)
    dist.all_reduce(tot)
    res = {"rank": R, "bits": [_bits(p) for p in net.parameters()], "w_loss": (tot / (b * W)).tolist(),
           "w_params": [p.detach().double().sum().item() for p in net.parameters()],
           "lr_next": eng.current_lr(), "steps": eng.lr_step_count()}
    if R == 0:
        cat = torch.cat([torch.cat([shards[r][k * b:(k + 1) * b] for r in range(W)]) for k in range(n_steps)])
        ref_net = build_net(seed=3, device=dev)
        ref = LeNetTrainStep(ref_net, batch_size=b * W, lr_schedule=lrs, **kw)
        res["one_loss"] = [x / (b * W) for x in train(ref, cat)]
        res["one_params"] = [p.detach().double().sum().item() for p in ref_net.parameters()]
        # the same run with the rate frozen at the constructor's: the schedule is what both runs follow
        flat_net = build_net(seed=3, device=dev)
        train(LeNetTrainStep(flat_net, batch_size=b * W, **kw), cat)
        res["frozen_params"] = [p.detach().double().sum().item() for p in flat_net.parameters()]
        res["max_abs_diff"] = [float((p.double() - q.double()).abs().max()) for p, q in
                               zip(net.parameters(), ref_net.parameters())]
        res["max_update"] = [float((q.double() - p0.double()).abs().max()) for q, p0 in
                             zip(ref_net.parameters(), net0)]
        res["max_param"] = [float(q.double().abs().max()) for q in ref_net.parameters()]
    emit(res)
    dist.destroy_process_group()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
