"""Counter-based dropout RNG: device state that advances in stream order, and the CPU definition of
the masks the HIP kernels draw (``csrc/include/pde_rng.h`` -- the addressing is fixed there).

A mask is a pure function of ``(seed, stream, draw number, site, position)`` through Philox4x32-10, so
nothing about it is stored: the forward, the backward and the ``dropout_mask`` debug kernel regenerate
the same bits from a 16-byte *snapshot* ``{seed lo, seed hi, draw, stream}``.  ``DeviceRNG.next()``
writes that snapshot and bumps the draw number with one tiny kernel and no host read, so a captured
training step draws fresh masks on every hipGraph replay.

The CPU path of every op that drops (``ops/transformer.py``) takes its mask from the numpy
implementation below: a CPU fp32 model and a GPU bf16 model with one seed drop the same elements.
"""
from __future__ import annotations

import numpy as np
import torch

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

SITE_KINDS = ("elementwise", "attention")


def philox4x32_10(counter, key):
    """Philox4x32-10 over arrays: ``counter`` = 4 and ``key`` = 2 integers or integer arrays (32-bit
    values, broadcast together); returns the 4 output words as uint32 arrays."""
    c = [np.asarray(x).astype(np.uint64) & _LO for x in counter]
    k0, k1 = (int(x) & 0xFFFFFFFF for x in key)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def threshold(p: float, site_kind: str = "elementwise") -> int:
    """Integer drop threshold: an element is kept iff its random word (byte) is >= this value."""
    if site_kind not in SITE_KINDS:
        raise ValueError(f"site_kind must be one of {SITE_KINDS}, got {site_kind!r}")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    return int(p * (4294967296.0 if site_kind == "elementwise" else 256.0))


def effective_p(p: float, site_kind: str = "elementwise") -> float:
    """The drop probability actually realised (and used by the 1 / keep scale): ``floor(p 2^32) / 2^32``
    at elementwise sites, ``floor(256 p) / 256`` at attention sites (8-bit threshold)."""
    return threshold(p, site_kind) / (4294967296.0 if site_kind == "elementwise" else 256.0)


def inv_keep(p: float, site_kind: str = "elementwise") -> float:
    return 1.0 / (1.0 - effective_p(p, site_kind))


def snapshot_words(snapshot):
    """(seed lo, seed hi, draw, stream) of a snapshot / state tensor as Python ints (a host read)."""
    if tuple(snapshot.shape) != (4,) or snapshot.dtype != torch.int32:
        raise ValueError("an RNG snapshot is an int32 tensor of 4 words")
    return tuple(int(v) & 0xFFFFFFFF for v in snapshot.tolist())


def _words(snapshot, site, groups):
    lo, hi, draw, stream = snapshot_words(snapshot)
    if not 0 <= int(site) < 65536:
        raise ValueError(f"site must fit 16 bits, got {site}")
    g = np.asarray(groups, dtype=np.uint64)
    return philox4x32_10((g & _LO, g >> _S32, draw, int(site) | ((stream & 0xFFFF) << 16)), (lo, hi))


def elementwise_mask(snapshot, site: int, numel: int, p: float):
    """uint8 keep-mask (1 = kept) of an elementwise site, flat ``[numel]``, on the CPU."""
    ngrp = (numel + 3) // 4
    w = np.stack(_words(snapshot, site, np.arange(ngrp, dtype=np.uint64)), axis=1).reshape(-1)[:numel]
    return torch.from_numpy((w >= np.uint32(threshold(p, "elementwise"))).astype(np.uint8))


def attention_mask(snapshot, site: int, B: int, H: int, T: int, p: float):
    """uint8 keep-mask ``[B, H, T(query), T(key)]`` of an attention site, on the CPU (T % 4 == 0)."""
    if T % 4:
        raise ValueError("attention masks need T % 4 == 0")
    t4 = T // 4
    w = np.stack(_words(snapshot, site, np.arange(B * H * t4 * t4, dtype=np.uint64)), axis=1)   # [G, word = q & 3]
    shifts = np.arange(4, dtype=np.uint32) * np.uint32(8)
    by = (w[:, :, None] >> shifts[None, None, :]) & np.uint32(0xFF)                             # [G, q & 3, k & 3]
    keep = (by >= np.uint32(threshold(p, "attention"))).astype(np.uint8)
    keep = keep.reshape(B, H, t4, t4, 4, 4).transpose(0, 1, 2, 4, 3, 5).reshape(B, H, T, T)
    return torch.from_numpy(np.ascontiguousarray(keep))


def dropout_mask(snapshot, site: int, p: float, shape=None, bht=None):
    """The keep-mask a kernel would draw, as uint8 on the snapshot's device: ``shape`` for an
    elementwise site, ``bht = (B, H, T)`` for an attention site (-> ``[B, H, T, T]``).  On the GPU this
    runs the ``dropout_mask`` debug kernel; it exists for tests and is never called by the model."""
    if (shape is None) == (bht is None):
        raise ValueError("give exactly one of shape (elementwise site) and bht (attention site)")
    if bht is not None:
        B, H, T = (int(v) for v in bht)
        if not snapshot.is_cuda:
            return attention_mask(snapshot, site, B, H, T, p)
        from .._ext import kernels
        out = torch.empty(B, H, T, T, device=snapshot.device, dtype=torch.uint8)
        kernels().dropout_mask(snapshot, int(site), threshold(p, "attention"), out, True)
        return out
    shape = tuple(int(v) for v in (shape if hasattr(shape, "__len__") else (shape,)))
    numel = int(np.prod(shape)) if shape else 1
    if not snapshot.is_cuda:
        return elementwise_mask(snapshot, site, numel, p).view(shape)
    from .._ext import kernels
    out = torch.empty(shape, device=snapshot.device, dtype=torch.uint8)
    kernels().dropout_mask(snapshot, int(site), threshold(p, "elementwise"), out, False)
    return out


class DeviceRNG:
    """Dropout RNG state ``{seed, draw number, stream}`` as a small device tensor.

    ``next()`` returns a fresh snapshot tensor for one training forward and increments the draw number
    on the device, in stream order and without a host read (capturable).  Every dropout site of that
    forward and of its backward reads the snapshot, which the autograd nodes keep alive: a second
    forward issued before the first backward cannot change the first one's masks.  ``stream`` is the
    data-parallel rank, so replicas with one seed drop different elements.  Not a module buffer:
    checkpoint it with ``state_dict()`` / ``load_state_dict()``."""

    def __init__(self, seed: int = 0, stream: int = 0, device=None):
        self.device = torch.device("cpu" if device is None else device)
        self.state = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._set(seed, 0, stream)

    def _set(self, seed, draw, stream):
        seed, draw, stream = int(seed), int(draw), int(stream)
        if not 0 <= stream < 65536:
            raise ValueError(f"stream must fit 16 bits, got {stream}")
        if not 0 <= draw < 2 ** 32:
            raise ValueError(f"draw number must fit 32 bits, got {draw}")
        self.seed, self.stream = seed & (2 ** 64 - 1), stream
        words = np.array([self.seed & 0xFFFFFFFF, self.seed >> 32, draw, stream], dtype=np.uint32).view(np.int32)
        self.state.copy_(torch.from_numpy(words.copy()))

    def manual_seed(self, seed: int, stream: int = None):
        """Reset: new seed, draw number 0 (and a new stream if given)."""
        self._set(seed, 0, self.stream if stream is None else stream)
        return self

    def next(self):
        snap = torch.empty_like(self.state)
        if self.state.is_cuda:
            from .._ext import kernels
            kernels().rng_next(self.state, snap)
        else:
            snap.copy_(self.state)
            draw = (snapshot_words(self.state)[2] + 1) & 0xFFFFFFFF
            self.state[2] = draw - (1 << 32) if draw >= 1 << 31 else draw     # stored as int32 bits
        return snap

    def draw_number(self) -> int:
        """Forwards drawn so far (a host sync)."""
        return snapshot_words(self.state)[2]

    def state_dict(self):
        return {"seed": self.seed, "draw": self.draw_number(), "stream": self.stream}

    def load_state_dict(self, sd):
        self._set(sd["seed"], sd["draw"], sd["stream"])

    def to(self, device):
        device = torch.device(device)
        if device != self.state.device:
            self.state = self.state.to(device)
            self.device = device
        return self
