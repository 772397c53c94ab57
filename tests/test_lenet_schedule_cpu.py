"""The toy-CNN engine's communication schedule as a value: ``Schedule`` labels round-trip, bad labels
are rejected, and ``schedule_candidates`` / ``set_schedule`` work from them (no GPU: both methods are
called on stand-ins that carry only the attributes they may touch)."""
import types

import pytest
import torch

from pytorch_distributed_example_amd.engine.lenet import MODES, LeNetTrainStep, Schedule

N_FC, N_CONV = 405632, 25664          # the engine's two gradient buckets (comm-path layout)
N_ALL = N_FC + N_CONV

DOCUMENTED = ["serial 431296:peer1", "overlap2 25664:peer1,405632:rccl", "serial 431296:pfold",
              "fused 25664:adam2,405632:peer2", "none"]


def _fake(peer, **extra):
    group = types.SimpleNamespace(rccl=object())          # an RCCL stand-in: only "is not None" is asked
    comm = types.SimpleNamespace(group=group, peer=peer, routes={})
    meta = lambda n: torch.empty(n, device="meta")
    return types.SimpleNamespace(comm=comm, optimizer="adam", grads=meta(N_ALL),
                                 bucket_grads=[meta(N_FC), meta(N_CONV)], **extra)


@pytest.mark.parametrize("label", DOCUMENTED)
def test_label_round_trip(label):
    sched = Schedule.parse(label)
    assert sched.label() == label
    assert sched.mode in MODES and sched == Schedule(sched.mode, sched.routes)


def test_parse_gives_mode_routes_and_properties():
    mode, routes = Schedule.parse("overlap2 25664:peer1,405632:rccl")      # unpacks like the old pair
    assert mode == "overlap2" and routes == {25664: "peer1", 405632: "rccl"}
    assert Schedule.parse("overlap 25664:rccl,405632:rccl")[0] == "overlap"
    assert Schedule(mode, routes).uses_peer and Schedule(mode, routes).cross_stream
    rccl_serial = Schedule.parse("serial 431296:rccl")
    assert not rccl_serial.uses_peer and not rccl_serial.cross_stream
    assert Schedule("fused", {N_FC: "peer2", N_CONV: "rccl"}).uses_peer
    assert [m for m in MODES if Schedule(m, {}).cross_stream] == ["overlap", "overlap2", "flat"]
    # pairs are sorted by numel whatever the order they were given in
    assert Schedule("overlap", {405632: "rccl", 25664: "peer2"}).label() == "overlap 25664:peer2,405632:rccl"


@pytest.mark.parametrize("label", ["", "overlap3 1:rccl", "Serial 431296:rccl", "serial 431296", "serial :rccl",
                                   "serial 431296:", "serial x:rccl", "serial 431296:rccl,oops",
                                   "overlap 25664=rccl"])
def test_parse_rejects(label):
    with pytest.raises(ValueError):
        Schedule.parse(label)


def test_candidates_without_peer_are_rccl_only():
    # no pfold_ok / world on the stand-in: without a peer they must not be touched
    cands = LeNetTrainStep.schedule_candidates(_fake(peer=None))
    assert cands and all(isinstance(c, Schedule) for c in cands)
    assert all(not c.uses_peer and c.mode != "fused" and set(c.routes.values()) == {"rccl"} for c in cands)
    labels = [c.label() for c in cands]
    assert len(set(labels)) == len(labels)
    assert all(m != "fused" and set(r.values()) == {"rccl"} for m, r in cands)      # still plain pairs


def test_candidates_with_peer():
    fake = _fake(peer=object(), pfold_ok=lambda two=False: True, world=2)
    cands = LeNetTrainStep.schedule_candidates(fake)
    flags = [c.uses_peer for c in cands]
    assert flags == sorted(flags) and not flags[0] and flags[-1]          # RCCL-only schedules first
    assert [c.label() for c in cands[-4:]] == [f"fused {N_CONV}:{b},{N_FC}:{a}" for a in ("peer1", "peer2")
                                               for b in ("adam1", "adam2")]
    # the rule of schedule_candidates' docstring, written out
    routes = ["rccl", "peer1", "peer2"]
    want = {f"{m} {N_CONV}:{b},{N_FC}:{a}" for m in ("overlap", "overlap2") for a in routes for b in routes}
    want |= {f"flat {N_ALL}:{a}" for a in routes} | {f"serial {N_ALL}:{a}" for a in routes + ["pfold", "pfold2"]}
    want |= {f"fused {N_CONV}:{b},{N_FC}:{a}" for a in ("peer1", "peer2") for b in routes + ["adam1", "adam2"]}
    labels = [c.label() for c in cands]
    assert len(labels) == len(set(labels)) == 36 and set(labels) == want
    assert all(Schedule.parse(s) == c for s, c in zip(labels, cands))


def test_set_schedule_sets_mode_and_routes_and_drops_graphs():
    fake = types.SimpleNamespace(comm=types.SimpleNamespace(routes={1: "stale"}), graphs={("k",): object()},
                                 mode="overlap")
    LeNetTrainStep.set_schedule(fake, "fused 25664:adam2,405632:peer2")
    assert fake.mode == "fused" and fake.comm.routes == {25664: "adam2", 405632: "peer2"}
    assert isinstance(fake.mode, str) and type(fake.comm.routes) is dict and fake.graphs == {}
    with pytest.raises(ValueError):
        LeNetTrainStep.set_schedule(fake, "sideways 1:rccl")
    assert fake.mode == "fused"                     # a rejected label changes nothing
