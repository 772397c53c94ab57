"""Muon on the CPU: the Newton-Schulz twin against the plain fp64 iteration, MuonMaster's validation,
GPT.muon_groups()."""
import pytest
import torch

from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.optim import MuonMaster


@pytest.mark.parametrize("shape", [(64, 128), (192, 320), (320, 192), (128, 512)])
def test_twin_against_fp64_and_singular_values(shape):
    torch.manual_seed(shape[0] + shape[1])
    x = torch.randn(*shape).bfloat16()
    twin, ref = ops.newton_schulz_reference(x), ops.newton_schulz_reference(x, emulate=False)
    assert twin.dtype == torch.bfloat16 and twin.shape == x.shape and ref.dtype == torch.float64
    assert torch.equal(ops.newton_schulz([x])[0], twin)            # CPU tensors run the twin
    # 15 bf16 roundings of ~2^-9 relative each, amplified by the iteration's slope (<= a = 3.4445) near zero
    assert ((twin.double() - ref).norm() / ref.norm()).item() < 0.03
    for o in (twin.double(), ref):
        s = torch.linalg.svdvals(o)
        assert 0.6 <= s.min().item() and s.max().item() <= 1.25, (s.min().item(), s.max().item())


def test_muon_master_validation():
    w = torch.nn.Parameter(torch.zeros(64, 128, dtype=torch.bfloat16))
    for bad in (torch.zeros(128), torch.zeros(2, 64, 64), torch.zeros(64, 96)):
        with pytest.raises(ValueError):
            MuonMaster([w, torch.nn.Parameter(bad.bfloat16())])
    with pytest.raises(ValueError):
        MuonMaster([w], ns_steps=-1)
    with pytest.raises(ValueError):                                  # one lr for all groups
        MuonMaster([{"params": [w], "lr": 0.1}, {"params": [torch.nn.Parameter(w.detach().clone())], "lr": 0.2}])
    with pytest.raises(ValueError):
        ops.muon.check_matrices([torch.zeros(64, 64)], "fp32")


def test_muon_groups_partition():
    cfg = GPTConfig(block_size=64, vocab_size=256, padded_vocab=256, n_layer=3, n_head=2, n_embd=64)
    m = build_gpt2(cfg, seed=0, device="cpu")
    mats, rest = m.muon_groups()
    assert len(mats) == 4 * cfg.n_layer and all(p.dim() == 2 for p in mats)
    assert sorted(tuple(p.shape) for p in mats[:4]) == sorted([(192, 64), (64, 64), (256, 64), (64, 256)])
    ids = [id(p) for p in mats + rest]
    assert len(set(ids)) == len(ids) and set(ids) == {id(p) for p in m.parameters()}
    assert any(p is m.transformer.wte.weight for p in rest) and any(p is m.transformer.wpe.weight for p in rest)
