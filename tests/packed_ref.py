"""Document layouts, their bounds written as Python loops, the document mask and the "needle outside" score
family for the packed-sequence tests (``test_packed_attention_cpu.py`` / ``test_packed_attention_gpu.py``).
Plain torch on the CPU; the attention side builds on ``attention_ref.py``."""
import math

import torch

import attention_ref as A


def ids_from_starts(T, starts):
    """int64 ``[T]`` document ids of one row whose documents begin at ``starts`` (ascending, first one 0).
    The ids alternate between two values only: a boundary is a change of id, not a new id."""
    assert starts[0] == 0 and list(starts) == sorted(set(starts)) and starts[-1] < T, starts
    ids = torch.zeros(T, dtype=torch.int64)
    for n, s in enumerate(starts):
        ids[s:] = 7 if n % 2 else 3
    return ids


def doc_ids(T, rows):
    """``[B, T]`` ids of a batch, ``rows`` = one list of starts per batch row."""
    return torch.stack([ids_from_starts(T, s) for s in rows])


def loop_bounds(ids):
    """``(doc_start, doc_end)`` as int32 ``[B, T]``, by the definition: a document begins at ``t = 0`` and
    wherever ``ids[b, t] != ids[b, t - 1]``."""
    B, T = ids.shape
    start = torch.zeros(B, T, dtype=torch.int32)
    end = torch.zeros(B, T, dtype=torch.int32)
    for b in range(B):
        row = ids[b].tolist()
        s = 0
        for t in range(T):
            if t > 0 and row[t] != row[t - 1]:
                s = t
            start[b, t] = s
        e = T - 1
        for t in range(T - 1, -1, -1):
            end[b, t] = e
            if t > 0 and row[t] != row[t - 1]:
                e = t - 1
    return start, end


def allowed_mask(start):
    """bool ``[B, 1, T(query), T(key)]``: ``start[b, q] <= k <= q``, written as loops over the documents."""
    B, T = start.shape
    out = torch.zeros(B, 1, T, T, dtype=torch.bool)
    for b in range(B):
        for q in range(T):
            out[b, 0, q, int(start[b, q]):q + 1] = True
    return out


# Layouts of the kernel tests: name -> starts of batch row b (b = 0, 1) for a row of T >= 256 positions.
#   one      a single document (the DOC kernels must agree with the plain ones)
#   mid200   a boundary strictly inside a 64-key tile and in the second half of a 128-query block: queries
#            200 .. 255 meet the tile 128 .. 191 with every key masked before their first visible key
#   tiles    boundaries exactly at 64 and 128 (and one document of 63, one of 65 positions in row 1)
#   len1     a document of length 1 (mid-tile, and at the first position of a tile in row 1)
#   span     a document that starts mid-block and spans more than one 128-query block
LAYOUTS = {
    "one": lambda T: [[0], [0]],
    "mid200": lambda T: [[0, 200], [0, 70, 200, 201 + (T - 256)]],
    "tiles": lambda T: [[0, 64, 128], [0, 63, 128, 193]],
    "len1": lambda T: [[0, 100, 101], [0, 64, 65, T - 1]],
    "span": lambda T: [[0, 50, T - 56], [0, 127, T - 1]],
}


def layout(name, B, T):
    return doc_ids(T, LAYOUTS[name](T)[:B])


def needle_outside(start):
    """Score about 40 on key ``doc_start[q] - 1``, the last key of the previous document (about N(0, 5)
    elsewhere): ``q[t] = a u[doc_start[t] - 1]``, ``k[t] = a u[t]`` with random unit vectors ``u`` and
    ``a^2 * scale = 40``; queries of a row's first document keep random directions.  The rows of v are
    random directions of length 8, as in ``attention_ref._peak_at``.  A mask that lets the previous
    document's last key through moves the row by about its whole magnitude."""
    def f(B, H, T, seed):
        g = torch.Generator().manual_seed(int(seed))
        u = A._units(g, B, H, T, A.HD)
        other = A._units(g, B, H, T, A.HD)
        src = (start.long() - 1)[:, None, :, None].expand(B, H, T, A.HD)        # [B, H, T, 64] gather index
        has = (src >= 0)
        qd = torch.where(has, u.gather(2, src.clamp_min(0)), other)
        return A._bf(A.PEAK * qd, A.PEAK * u, math.sqrt(A.HD) * A._units(g, B, H, T, A.HD))
    return f


def make(family, start, B, H, T, seed=0):
    """bf16 ``q, k, v, dO`` ``[B, H, T, 64]``: ``gauss1`` of ``attention_ref`` or ``needle_outside``."""
    if family == "needle_outside":
        q, k, v = needle_outside(start)(B, H, T, seed)
        dO = torch.randn(B, H, T, A.HD, generator=torch.Generator().manual_seed(seed + 7919), dtype=A.F64).to(A.BF16)
        return q, k, v, dO
    return A.make(family, B, H, T, seed)
