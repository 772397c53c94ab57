"""Distributed plumbing on CPU (survey §4 items 4/7): native store, host collectives, dist API,
process groups, launcher failure handling -- W in {2, 3, 4} processes on 127.0.0.1."""
import threading
import time
from types import SimpleNamespace

import pytest

from _mp import run_ranks
from pytorch_distributed_example_amd._ext import runtime
from pytorch_distributed_example_amd.launch import free_port


def test_store_basic():
    rt = runtime()
    srv = rt.StoreServer("127.0.0.1", 0)
    a = rt.StoreClient("127.0.0.1", srv.port, 5000)
    b = rt.StoreClient("127.0.0.1", srv.port, 5000)
    a.set("k", b"v1")
    assert b.get("k") == b"v1"
    assert a.add("ctr", 3) == 3 and b.add("ctr", 4) == 7
    assert b.check(["k", "ctr"]) and not b.check(["nope"])
    got = {}

    def waiter():
        got["v"] = b.get("late")

    t = threading.Thread(target=waiter)
    t.start()
    time.sleep(0.2)
    a.set("late", b"x")
    t.join(5)
    assert got.get("v") == b"x"
    # compare_set: missing key + empty expected -> set; wrong expected -> unchanged
    assert a.compare_set("cas", b"", b"first") == b"first"
    assert a.compare_set("cas", b"zzz", b"second") == b"first"
    assert a.compare_set("cas", b"first", b"second") == b"second"
    n = a.num_keys()
    assert a.delete_key("k")
    assert a.num_keys() == n - 1
    b.timeout_ms = 300
    with pytest.raises(Exception):
        b.get("never-set")
    b.timeout_ms = 5000
    a.set("after-timeout", b"ok")
    assert b.get("after-timeout") == b"ok"      # client recovers after a timed-out request
    srv.stop()


@pytest.mark.parametrize("world", [2, 3])
def test_collectives_env(world):
    rc, res, logs = run_ranks("collectives", world, "gloo", "env")
    assert rc == 0, logs
    assert all(r and r["ok"] for r in res)


def test_collectives_tcp_w4():
    rc, res, logs = run_ranks("collectives", 4, "gloo", "tcp")
    assert rc == 0, logs
    assert all(r and r["ok"] for r in res)


@pytest.mark.parametrize("world", [2, 3])
def test_host_p2p_large_exchange(world):
    rc, res, logs = run_ranks("p2p_large", world, "8")
    assert rc == 0, logs
    assert all(r and r["ok"] for r in res)


@pytest.mark.parametrize("end", ["barrier", "destroy"])
def test_host_isend_unwaited_still_delivered(end):
    t0 = time.time()
    rc, res, logs = run_ranks("p2p_unwaited", 2, end)
    assert rc == 0, logs
    assert all(r and r["ok"] for r in res)
    assert time.time() - t0 < 60


@pytest.mark.parametrize("world", [2, 4])
def test_groups_and_toy_pattern(world):
    rc, res, logs = run_ranks("groups", world)
    assert rc == 0, logs
    assert all(r and r["ok"] for r in res)


def test_launcher_terminates_gang_on_failure():
    t0 = time.time()
    rc, _, logs = run_ranks("fail", 3)
    assert rc == 3, logs
    assert time.time() - t0 < 60


def test_rank_none_error():
    from pytorch_distributed_example_amd import dist
    with pytest.raises((ValueError, TypeError), match="rank must be an integer"):
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{free_port()}", rank=None, world_size=2)


def test_tcp_port_zero_single_process():
    """tcp://host:0 at world size 1: the store binds an ephemeral port itself (bench.py's W = 1 comm
    figure; a probed free port was once taken between probe and bind).  Refused for world size > 1."""
    import torch

    from pytorch_distributed_example_amd import dist
    with pytest.raises(ValueError, match="port 0 needs world_size 1"):
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:0", rank=0, world_size=2)
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:0", rank=0, world_size=1)
    try:
        t = torch.tensor([3.0, 4.0])
        dist.all_reduce(t)
        assert t.tolist() == [3.0, 4.0]
    finally:
        dist.destroy_process_group()
    assert not dist.is_initialized()


@pytest.mark.parametrize("world", [2, 3])
def test_torch_distributed_backend_pde(world):
    """torch.distributed with backend="pde" (the framework runtime registered as a c10d backend):
    reference-style toy loop, collectives and torch's own DDP, on the CPU host collectives."""
    rc, res, logs = run_ranks("torch_backend", world, "cpu")
    assert rc == 0, "\n".join(logs)
    assert all(r["sums"] == res[0]["sums"] for r in res)


def test_bench_w2_forced_peer_failure_degrades_to_rccl():
    """Verdict r1 item 4: a peer-path failure on one rank leaves every rank on RCCL-only routes and
    schedules, reported in the bench JSON fields, within a bounded time."""
    t0 = time.time()
    rc, res, logs = run_ranks("bench_peer_fail", 2, extra_env={"PDE_PEER_FORCE_FAIL": "1"})
    assert rc == 0, logs
    assert all(r and r["ok"] for r in res), logs
    assert "forced" in res[1]["reason"] and res[0]["reason"]          # rank 0 learns it from the vote
    assert time.time() - t0 < 90


def test_bench_failure_prints_one_json_line_w2():
    """bench.py at W=2 where the step cannot run (no GPU here): rank 0 still prints exactly one JSON
    line (value null + error), every rank exits non-zero, bounded time."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t0 = time.time()
    for attempt in range(2):     # a free_port() race with another process ends the rendezvous, not the bench
        p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "bench.py", "--gpus",
                            "2", "--steps", "4", "--warmup", "1"], cwd=root, capture_output=True, text=True,
                           timeout=240, env={**os.environ, "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""})
        lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
        if lines or "EADDRINUSE" not in p.stderr and "address already in use" not in p.stderr.lower():
            break
    assert p.returncode != 0
    assert len(lines) == 1, p.stdout + p.stderr
    out = json.loads(lines[0])
    assert out["value"] is None and out["n_gpus"] == 2 and out["error"]
    assert time.time() - t0 < 480


def test_bench_self_launches_n_ranks_without_torchrun():
    """Verdict r2 item 1: ``python bench.py --gpus 4`` with no launcher starts 4 rank processes itself
    (never a silent 1-GPU run labelled otherwise) and relays exactly one JSON line carrying n_gpus 4
    (the error line here: no GPU), with a non-zero exit code."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--steps", "4", "--warmup", "1"], cwd=root,
                       capture_output=True, text=True, timeout=240, env=env)
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout + p.stderr
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["value"] is None and out["error"]
    assert p.returncode != 0
    started = {l.split()[2] for l in p.stderr.splitlines() if l.startswith("[bench] rank ")}
    assert started == {"0/4", "1/4", "2/4", "3/4"}, p.stderr


def test_bench_refuses_world_size_mismatch():
    """A launch whose WORLD_SIZE differs from --gpus prints one error line and exits 2."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "8"], cwd=root, capture_output=True, text=True,
                       timeout=120, env=env)
    assert p.returncode == 2
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["value"] is None and "WORLD_SIZE=1" in out["error"] and out["n_gpus"] == 1


@pytest.mark.parametrize("world,fail_rank", [(2, "1"), (4, "2")])
def test_bench_forced_peer_failure_on_one_rank_is_collective(world, fail_rank):
    """Verdict r4 item 1: a peer-setup failure injected on ONE rank of W leaves EVERY rank on
    RCCL-only routes and schedules (the set-up vote is collective), reported with a reason."""
    rc, res, logs = run_ranks("bench_peer_fail", world, extra_env={"PDE_PEER_FORCE_FAIL": fail_rank})
    assert rc == 0, logs
    assert all(r and r["ok"] for r in res), logs
    assert "forced" in res[int(fail_rank)]["reason"]
    assert all(r["reason"] for r in res)


def _bench_stub(world, extra_env=None):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PDE_BENCH_STUB="1", **(extra_env or {}))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--steps", "20",
                        "--warmup", "5", "--no-spin-wait"], capture_output=True, text=True, env=env, timeout=180)
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, (p.stdout, p.stderr[-2000:])
    return p.returncode, json.loads(lines[0])


@pytest.mark.parametrize("world", [2, 3])
def test_bench_multi_rank_line_carries_anchor_and_rank_devices(world):
    """Verdict r4 item 1c: ``bench.py --gpus N`` (self-launched, CPU stub engine) emits ONE line with
    the same-job W=1 anchor, ``scaling_eff_same_job`` and every rank's device row."""
    rc, d = _bench_stub(world)
    assert rc == 0, d
    assert d["n_gpus"] == world and d["value"] > 0
    assert [r["rank"] for r in d["per_rank"]] == list(range(world))
    assert len({r["device_id"] for r in d["per_rank"]}) == world
    assert len(d["w1_anchor_per_rank"]) == world and d["w1_anchor_images_per_s"] > 0
    assert abs(d["scaling_eff_same_job"] - d["value"] / world / d["w1_anchor_images_per_s"]) < 1e-3
    assert d["data"].startswith("STUB")


def test_bench_multi_rank_repeated_device_fails():
    """Every rank reporting the same GPU (the reference's all-on-GPU-0 bug, mnist/main.py:181-182)
    makes the run fail with an error line instead of a number."""
    rc, d = _bench_stub(2, {"PDE_BENCH_STUB_DEV": "gpu-0"})
    assert rc != 0 and d["value"] is None
    assert "share one GPU" in d["error"]


def test_bench_validate_ranks_rules():
    import bench
    row = lambda r, **k: dict({"rank": r, "host": "h", "device": r, "device_id": f"u{r}", "rccl_world": 4,
                               "rccl_device": r, "peer_ok": True}, **k)
    good = [row(r) for r in range(4)]
    assert bench.validate_ranks(good, 4) == ""
    assert "share one GPU" in bench.validate_ranks([row(0), row(1, device_id="u0"), row(2), row(3)], 4)
    assert bench.validate_ranks([row(0), row(1, device_id="u0"), row(2), row(3)], 4, shared_gpu=True) == ""
    assert "3 ranks, not 4" in bench.validate_ranks([row(0), row(1), row(2, rccl_world=3), row(3)], 4)
    assert "on device 0" in bench.validate_ranks([row(0), row(1, rccl_device=0), row(2), row(3)], 4)
    assert "some ranks only" in bench.validate_ranks([row(0), row(1, peer_ok=False), row(2), row(3)], 4)
    assert "expected 4" in bench.validate_ranks(good[:3], 4)


def test_bench_replay_plan():
    """The timed window's graph replays: exactly n steps, the lead step(s) first, every length primed
    (the set bench.py captures before the warm-up: S, the warm-up graph, the timed remainder, 1)."""
    import bench
    assert bench._replay_plan(20, 20, 1) == [1, 19]
    assert bench._replay_plan(20, 20, 0) == [20]
    assert bench._replay_plan(5, 5, 0) == [5]
    assert bench._replay_plan(2000, 100, 1) == [1] + [100] * 19 + [99]
    assert bench._replay_plan(1, 1, 1) == [1]
    for n in (1, 7, 20, 64, 2000):
        for L in (0, 1, 2):
            L = min(L, n)
            S = bench._graph_steps(SimpleNamespace(graph_steps=0, steps=n))
            plan = bench._replay_plan(n, S, L)
            assert sum(plan) == n and plan[:L] == [1] * L
            assert set(plan) <= {S, (n - L) % S or 1, 1}


def test_bench_secondary_figure_only_with_full():
    """A plain run measures the headline alone: the W=1 comm figure belongs to ``--full`` (or to an
    explicit ``--comm-figure on``), never to W > 1 and never to an automatic ``--force-comm`` run."""
    import bench
    parse = lambda *a: bench.build_parser().parse_args(list(a))
    assert not bench.comm_figure_wanted(parse("--gpus", "1", "--steps", "20", "--warmup", "5"), 1)
    assert bench.comm_figure_wanted(parse("--full"), 1)
    assert bench.comm_figure_wanted(parse("--comm-figure", "on"), 1)
    assert not bench.comm_figure_wanted(parse("--full", "--comm-figure", "off"), 1)
    assert not bench.comm_figure_wanted(parse("--full", "--force-comm"), 1)
    assert not bench.comm_figure_wanted(parse("--full", "--gpus", "2"), 2)
    import bench_models
    assert not bench_models._comm_figure_wanted(parse("--model", "gpt2"), 1)
    assert bench_models._comm_figure_wanted(parse("--model", "gpt2", "--full"), 1)
    assert bench_models._comm_figure_wanted(parse("--model", "gpt2", "--comm-figure", "on"), 1)
    assert not bench_models._comm_figure_wanted(parse("--model", "gpt2", "--full", "--comm-figure", "off"), 1)


def test_bench_dump_outputs_dtypes_cap_and_fixed_sample(tmp_path):
    """``--dump-outputs``: one .npy per name, float32 (float64 / integers as float64), everything
    within the byte cap, and an array above its share cut to the same seeded sample on every call."""
    import numpy as np
    import torch

    import bench
    big = torch.arange(1000, dtype=torch.float32) * 0.5
    arrays = {"w": big, "half": torch.ones(3, dtype=torch.bfloat16), "count": torch.tensor([7], dtype=torch.int64),
              "meter": torch.tensor([1.25], dtype=torch.float64)}
    n = bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert n == {"w": 1000, "half": 3, "count": 1, "meter": 1}
    assert got["w"].dtype == np.float32 and got["half"].dtype == np.float32
    assert got["count"].dtype == np.float64 and got["meter"].dtype == np.float64
    assert np.array_equal(got["w"], big.numpy()) and got["count"][0] == 7.0 and got["meter"][0] == 1.25
    # capped at 1600 bytes: 400 per array, so w keeps 100 of its 1000 elements, the small ones stay whole
    n = bench.dump_outputs(str(tmp_path / "b"), arrays, cap_bytes=1600)
    assert n == {"w": 100, "half": 3, "count": 1, "meter": 1}
    bench.dump_outputs(str(tmp_path / "c"), arrays, cap_bytes=1600)
    wb, wc = np.load(tmp_path / "b" / "w.npy"), np.load(tmp_path / "c" / "w.npy")
    assert wb.shape == (100,) and np.array_equal(wb, wc)
    assert np.all(np.diff(wb) > 0) and np.isin(wb, big.numpy()).all()      # distinct elements, in order
    assert sum(f.stat().st_size - 128 for f in (tmp_path / "b").iterdir()) <= 1600


def test_bench_stub_plain_run_dumps_and_reports_ms_per_step(tmp_path):
    """``bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`` (CPU stub engine): one result line
    with ``ms_per_step`` for the K timed steps, no secondary figure, and the meters written."""
    import json
    import os
    import subprocess
    import sys

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PDE_BENCH_STUB="1", PDE_BENCH_NUMA="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup",
                        "5", "--no-spin-wait", "--dump-outputs", str(tmp_path / "out")], capture_output=True,
                       text=True, env=env, timeout=180)
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert p.returncode == 0 and len(lines) == 1, (p.stdout, p.stderr[-2000:])
    d = json.loads(lines[0])
    assert d["steps"] == 20 and d["ms_per_step"] > 0 and "w1_rccl_comm" not in d
    assert abs(d["value"] - 128 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert sorted(os.listdir(tmp_path / "out")) == ["correct.npy", "loss_sum.npy"]
    assert np.load(tmp_path / "out" / "loss_sum.npy").dtype == np.float64
