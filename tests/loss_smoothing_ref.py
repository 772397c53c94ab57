"""The smoothed and weighted loss's definition written as Python loops over ``(b, t)`` and ``v`` in fp64, shared by
``test_loss_smoothing_cpu.py`` and ``test_loss_smoothing_gpu.py``.  Which rows count, and ``inv``, come from the
masked loss's loops (``masked_loss_ref.loop_targets``)::

    row_i         = w_i * (lse - (1 - eps) * x[t] - (eps / V) * sum_{v<V} x[v] + zc * lse^2)     valid(i), else 0
    loss          = inv * sum_i row_i
    dlogits[i, v] = w_i * inv * ((1 + 2 * zc * lse) * p[v] - (1 - eps) * [v == t] - eps / V)     v < V, valid(i)
"""
import math
from typing import NamedTuple

import torch

import masked_loss_ref as M


class LoopLoss(NamedTuple):
    rows: torch.Tensor        # fp64 [B, T]: row_i, 0 where not valid
    loss: float               # inv * sum of the rows
    dlogits: torch.Tensor     # fp64 [B, T, V]
    eff: torch.Tensor         # int64 [B, T]: the target where valid, else -1
    inv: float
    count: int
    mag: torch.Tensor         # fp64 [B, T, V]: w inv ((1 + 2 zc lse) p + (1 - eps) [v == t] + eps / V), the sum of
    #                           the magnitudes of dlogits' terms (what a rounding error is relative to)


def loop_loss(logits, targets, V, eps=0.0, zc=0.0, weights=None, **kw):
    """``logits`` ``[B, T, >= V]`` of any float dtype (read as fp64), ``targets`` int64 ``[B, T]``, ``weights``
    ``[B, T]`` or None; ``kw``: ``ignore_index``, ``loss_mask``, ``doc_end``, ``reduction``, ``denom`` of
    ``masked_loss_ref.loop_targets``.  A row that is not valid is never read, nor is its weight."""
    B, T = targets.shape
    eff, count, inv, _ = M.loop_targets(targets, V, **kw)
    inv = float(inv)
    rows = torch.zeros(B, T, dtype=torch.float64)
    d = torch.zeros(B, T, V, dtype=torch.float64)
    mag = torch.zeros(B, T, V, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            y = int(eff[b, t])
            if y < 0:
                continue
            w = 1.0 if weights is None else float(weights[b, t])
            x = logits[b, t, :V].double().tolist()
            m = max(x)
            lse = m + math.log(math.fsum(math.exp(xv - m) for xv in x))
            rows[b, t] = w * (lse - (1.0 - eps) * x[y] - (eps / V) * math.fsum(x) + zc * lse * lse)
            k = 1.0 + 2.0 * zc * lse
            kp = [k * math.exp(xv - lse) for xv in x]
            g = [w * inv * (kpv - eps / V) for kpv in kp]
            a = [abs(w * inv) * (abs(kpv) + eps / V) for kpv in kp]
            g[y] -= w * inv * (1.0 - eps)
            a[y] += abs(w * inv) * (1.0 - eps)
            d[b, t] = torch.tensor(g, dtype=torch.float64)
            mag[b, t] = torch.tensor(a, dtype=torch.float64)
    loss = inv * math.fsum(rows.reshape(-1).tolist())
    return LoopLoss(rows, loss, d, eff, inv, count, mag)
