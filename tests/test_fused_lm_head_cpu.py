"""On CPU tensors ``lm_head_loss(fused=True)`` is the call without the flag, and ``lm_head_stats`` is the definition."""
import pytest
import torch

from pytorch_distributed_example_amd.ops import transformer as TR


@pytest.mark.parametrize("kw", [{}, dict(ignore_index=-1, reduction="none"),
                                dict(ignore_index=-1, label_smoothing=0.1, z_loss=1e-4, reduction="sum")])
def test_cpu_ignores_fused(kw):
    g = torch.Generator().manual_seed(0)
    h, w = torch.randn(6, 16, generator=g), torch.randn(24, 16, generator=g)
    tg = torch.randint(0, 20, (6,), generator=g)
    if kw:
        tg[2] = -1
    assert TR.lm_head_loss(h, w, tg, 20, fused=True, **kw).equal(TR.lm_head_loss(h, w, tg, 20, **kw))
    lse, xt, sx = TR.lm_head_stats(h, w, tg, 20, with_sum=True)
    x = h @ w[:20].T
    ok = tg >= 0
    assert torch.allclose(lse[ok], torch.logsumexp(x, 1)[ok]) and torch.allclose(sx[ok], x.sum(1)[ok])
    assert torch.allclose(xt[ok], x[ok, tg[ok]]) and (lse[~ok] == 0).all() and (xt[~ok] == 0).all()
