"""The masked loss's definition written as Python loops over ``(b, t)``, and the option cases shared by
``test_masked_loss_cpu.py`` and ``test_masked_loss_gpu.py``.  Plain torch on the CPU; document layouts come from
``packed_ref.py``."""
import torch

import packed_ref as P


def loop_targets(targets, V, ignore_index=None, loss_mask=None, doc_end=None, reduction="mean", denom=None):
    """``(effective targets, count, inv, out_of_range)`` by the definition.  ``targets`` int64 ``[B, T]``,
    ``loss_mask`` ``[B, T]`` or None, ``doc_end`` int32 ``[B, T]`` (document ends are masked) or None.  ``inv`` is
    an fp32 tensor computed by torch's fp32 division."""
    B, T = targets.shape
    eff = torch.full((B, T), -1, dtype=torch.int64)
    count = oor = 0
    for b in range(B):
        for t in range(T):
            sel = loss_mask is None or int(loss_mask[b, t]) != 0
            if doc_end is not None and t < T - 1 and int(doc_end[b, t]) == t:
                sel = False
            y = int(targets[b, t])
            if not sel or (ignore_index is not None and y == ignore_index):
                continue
            if 0 <= y < V:
                eff[b, t] = y
                count += 1
            else:
                oor += 1
    if denom is not None:
        d = torch.tensor(float(denom), dtype=torch.float32)
        inv = 1.0 / d if float(d) > 0 else torch.zeros((), dtype=torch.float32)
    elif reduction == "mean":
        inv = 1.0 / torch.tensor(float(max(count, 1)), dtype=torch.float32)
    else:
        inv = torch.ones((), dtype=torch.float32)
    return eff, count, inv, oor


def make_case(name, B, T, V, seed=0):
    """One option combination: ``(targets [B, T], kwargs for the loops)``; ``doc_ids`` (or None) rides along under
    the key ``"doc_ids"`` and is turned into ``doc_end`` by the caller."""
    g = torch.Generator().manual_seed(seed)
    tg = torch.randint(0, V, (B, T), generator=g)
    drop = torch.rand(B, T, generator=g) < 0.4
    kw = {}
    if name == "ignore_neg":
        tg[drop] = -100
        kw = dict(ignore_index=-100)
    elif name == "ignore_token":            # a real token id: every occurrence is ignored, drawn or planted
        tg[drop] = 7
        kw = dict(ignore_index=7)
    elif name == "mask_bool":
        kw = dict(loss_mask=~drop)
    elif name == "mask_u8":
        kw = dict(loss_mask=(~drop).to(torch.uint8) * 3)     # any nonzero value selects
    elif name == "out_of_range":
        tg[drop] = V + 5
        tg.view(-1)[0] = -3
        tg.view(-1)[-1] = -100
        kw = dict(ignore_index=-100)
    elif name == "all_ignored":
        tg[:] = -100
        kw = dict(ignore_index=-100)
    elif name == "all_masked":
        kw = dict(loss_mask=torch.zeros(B, T, dtype=torch.bool))
    elif name == "everything":              # the three mechanisms and stray targets at once
        tg[drop] = -100
        tg[torch.rand(B, T, generator=g) < 0.05] = V
        kw = dict(ignore_index=-100, loss_mask=torch.rand(B, T, generator=g) < 0.7)
    elif name != "plain":
        raise KeyError(name)
    return tg, kw


CASES = ("plain", "ignore_neg", "ignore_token", "mask_bool", "mask_u8", "out_of_range", "all_ignored", "all_masked",
         "everything")


def doc_end_of(layout, B, T):
    """``(doc_ids, doc_end)`` of a ``packed_ref`` layout, the ends by its loops."""
    ids = P.layout(layout, B, T)
    return ids, P.loop_bounds(ids)[1]
