"""ResNet-18 bf16 benchmark (``python bench.py --model resnet18``): synthetic 3x224x224 images,
channels-last bf16, DDP over RCCL, fused BN+ReLU kernels, SGD(momentum 0.9, wd 5e-5) with fp32
master weights.  Metric: images/s for the whole node (weak scaling: fixed per-GPU batch)."""
from __future__ import annotations

import json

import bench_models
from bench_models import (_cap, _capture_step, _comm_figure_wanted, _dump, _graph_wanted, _setup, _timed, _tune,
                          _w1_comm_group)


def _resnet_run(args, torch, dist, rank, world, dev, comm):
    from pytorch_distributed_example_amd import ops
    from pytorch_distributed_example_amd.models import build_resnet18
    from pytorch_distributed_example_amd.optim import SGDMaster
    from pytorch_distributed_example_amd.parallel import DistributedDataParallel

    B = args.batch_size if args.batch_size != 128 else 256
    model = build_resnet18(seed=args.seed, device=dev)
    ddp = DistributedDataParallel(model, bucket_cap_mb=_cap(args), force_comm=world == 1) if comm else model
    opt = SGDMaster(model.decay_groups(5e-5), lr=0.1, momentum=0.9)
    # 8 batches per rank of class-conditional synthetic images, sharded by the DistributedSampler
    from pytorch_distributed_example_amd.data import DistributedSampler, synthetic_images
    pool = 8 * B * world
    sampler = DistributedSampler(range(pool), num_replicas=world, rank=rank, shuffle=True, seed=args.seed)
    X, Y = synthetic_images(sampler.indices_tensor().long(), seed=args.seed, device=dev)
    nb = X.shape[0] // B
    it = [0]
    losses = []

    ones = torch.ones((), device=dev, dtype=torch.float32)        # d loss / d loss (no fill kernel per step)

    def eager_step(x, y):
        opt.zero_grad()
        loss = ops.cross_entropy(ddp(x), y)       # bf16 logits straight into the CE kernel (no cast)
        loss.backward(ones)
        opt.step()
        return loss.detach()

    def step():
        i = it[0] % nb
        it[0] += 1
        losses.append(eager_step(X[i * B:(i + 1) * B], Y[i * B:(i + 1) * B]))

    extra = _tune(ddp, step, world, args,
                  restore=list(model.parameters()) + list(model.buffers()) + opt.state_tensors())
    if _graph_wanted(args):
        # the whole step (forward with the DDP buffer broadcast, loss, backward with the bucket
        # all-reduces, SGD with its flat fp32 master / momentum buffers) is captured once into a hipGraph
        # and replayed: ~230 kernel launches per step leave the host, and the ~0.3 ms of launch gaps with
        # them.  Each step copies its batch into the static input first (inside the timed region).
        # SGDMaster has no host-side step state, so a replay is exact.
        sx, sy = X[:B].clone(), Y[:B].clone()
        graph, static_loss = _capture_step(torch, eager_step, sx, sy)

        def step():                                  # noqa: F811 - the graph-replay step
            i = it[0] % nb
            it[0] += 1
            sx.copy_(X[i * B:(i + 1) * B])
            sy.copy_(Y[i * B:(i + 1) * B])
            graph.replay()
            losses.append(static_loss)

        graph.replay()                               # first launch of the graph outside the timed window
        extra["mode"] = "hipgraph (whole step" + (", DDP collectives captured)" if comm else ")")
    else:
        extra["mode"] = "eager"
    elapsed = _timed(torch, dist, world, step, args.warmup, args.steps)
    if comm:
        ddp.check_health()
    return {"elapsed": elapsed, "extra": extra, "B": B, "last_loss": float(losses[-1]), "model": model}


def bench_resnet18(args):
    torch, dist, rank, world, dev = _setup(getattr(args, "shared_gpu", False), getattr(args, "numa_bdf", None))
    r = _resnet_run(args, torch, dist, rank, world, dev, comm=world > 1 or getattr(args, "force_comm", False))
    B = r["B"]
    _dump(args, rank, r.pop("model"), r["last_loss"])
    ips = args.steps * B * world / r["elapsed"]
    out = {
        "metric": "images/sec (whole node), ResNet-18 bf16 DDP",
        "value": round(ips, 1), "unit": "images/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(r["elapsed"] / args.steps * 1e3, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic class-conditional 3x224x224 images (class prototype + noise), 8 batches per rank "
                "sharded by DistributedSampler, random-init weights",
        "config": {"model": "ResNet-18 (11.69M params, torchvision layout)", "global_batch": B * world,
                   "per_gpu_batch": B, "seq_len": None, "parallelism": f"dp{world}",
                   "host_cpus": f"NUMA node of GPU {bench_models._NUMA[0]}" if bench_models._NUMA[0] else "unpinned",
                   "optimizer": "SGD(0.1, momentum 0.9, wd 5e-5; fp32 master)", **r["extra"],
                   "memory_format": "channels_last"},
        "last_loss": round(r["last_loss"], 4),
    }
    if _comm_figure_wanted(args, world):
        try:
            _w1_comm_group(dist)
            r2 = _resnet_run(args, torch, dist, rank, world, dev, comm=True)
            out["w1_rccl_comm"] = {"value": round(args.steps * B / r2["elapsed"], 1),
                                   "ms_per_step": round(r2["elapsed"] / args.steps * 1e3, 3), **r2["extra"]}
        except Exception as e:   # noqa: BLE001 - the headline stands; report the secondary failure
            out["w1_rccl_comm"] = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        from pytorch_distributed_example_amd.utils.stdio import emit_result
        emit_result(out)
    if dist.is_initialized():
        dist.destroy_process_group()
