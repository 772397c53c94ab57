"""GPT-2 generation ops (bf16) over the HIP kernels of ``csrc/kernels/decode.hip``: skinny linear
(``M <= 16`` rows), KV cache with decode attention, decode embedding, and the device-side sampler with
its CPU twin.

Everything that changes from token to token -- position, output slot, RNG draw number, the rows'
"finished" flags -- lives in a small device buffer (``DecodeState``, layout in
``csrc/include/pde_decode.h``) that the kernels read and the sampler advances, so one decode step can be
captured once and replayed per token with no host work in between.

Sampling definition (``sample`` on the GPU and ``sample_reference`` in numpy compute the same thing):

* ``temperature == 0``: the lowest index attaining the row maximum over the first ``V`` columns.
* otherwise ``top_k = k`` keeps ``{v : logit_v >= k-th largest logit value of the row}`` -- ties at the
  threshold are kept, so the set can exceed ``k`` -- and the token is
  ``argmax_v(float(logit_v) * fp32(1 / temperature) + g_v)`` over that set, lowest index on ties, with the
  Gumbel noise ``g_v = -log(-log(u_v))``, ``u_v = ((w_v >> 9) + 0.5) * 2^-23`` and ``w_v`` word ``v & 3`` of
  Philox group ``b * ceil(Vp / 4) + (v >> 2)`` at site 0 of the snapshot (``ops/rng.py`` addressing).
  This is the Gumbel-max form of sampling from ``softmax(logits / temperature)``; one draw number per token.

GPU tensors always run the framework kernels; an unsupported shape raises ``NotImplementedError``.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from .._ext import kernels
from . import rng as R

_BF16 = torch.bfloat16

STATE_WORDS = 24          # pde_decode.h
_RNG, _POS, _STEP, _FIN = 0, 4, 5, 8
MAX_ROWS = 16


class DecodeState:
    """The device-side state of a generation: RNG words, position, step, finished flags (int32 x 24)."""

    def __init__(self, device=None, rng_state=None, pos: int = 0, step: int = 0):
        self.device = torch.device("cpu" if device is None else device)
        self.buf = torch.zeros(STATE_WORDS, dtype=torch.int32, device=self.device)
        self.reset(rng_state, pos, step)

    def reset(self, rng_state=None, pos: int = 0, step: int = 0):
        """Position / step from the host, RNG words copied from a ``DeviceRNG`` state or snapshot (a
        device-to-device copy: no host read); the finished flags are cleared."""
        init = torch.zeros(STATE_WORDS, dtype=torch.int32)
        init[_POS], init[_STEP] = int(pos), int(step)
        self.buf.copy_(init)
        if rng_state is not None:
            if tuple(rng_state.shape) != (4,) or rng_state.dtype != torch.int32:
                raise ValueError("an RNG state / snapshot is an int32 tensor of 4 words")
            self.buf[:4].copy_(rng_state)
        return self

    @property
    def rng(self):
        return self.buf[_RNG:_RNG + 4]

    @property
    def finished(self):
        return self.buf[_FIN:_FIN + MAX_ROWS]

    def pos(self) -> int:
        return int(self.buf[_POS].item())

    def step(self) -> int:
        return int(self.buf[_STEP].item())

    def advance_(self):
        """What the sampler's tail does, for the CPU definition of the ops."""
        self.buf[_POS] += 1
        self.buf[_STEP] += 1
        draw = (R.snapshot_words(self.rng)[2] + 1) & 0xFFFFFFFF
        self.buf[_RNG + 2] = draw - (1 << 32) if draw >= 1 << 31 else draw


# --------------------------------------------------------------------------------------- skinny linear
def skinny_linear(x, w, b=None, gelu: bool = False):
    """``y[M, N] = x[M, K] w[N, K]^T (+ b) (-> tanh-GELU)`` for decode: ``1 <= M <= 16``, ``K % 64 == 0``,
    ``N % 8 == 0``, bf16.  Every weight element is read once, straight into MFMA fragments; the result
    does not depend on block arrival order (two calls are bit-identical)."""
    if not x.is_cuda:
        y = F.linear(x, w, b)
        return F.gelu(y, approximate="tanh") if gelu else y
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise NotImplementedError(f"skinny_linear: x [M, K] and w [N, K] (got {tuple(x.shape)}, {tuple(w.shape)})")
    M, Kd = x.shape
    N = w.shape[0]
    if not 1 <= M <= MAX_ROWS:
        raise NotImplementedError(f"skinny_linear: 1 <= M <= {MAX_ROWS} rows (got {M}); use ops.transformer.linear")
    if Kd % 64 or N % 8:
        raise NotImplementedError(f"skinny_linear: in_features % 64 == 0 and out_features % 8 == 0 (got {Kd}, {N})")
    if x.dtype != _BF16 or w.dtype != _BF16 or (b is not None and b.dtype != _BF16):
        raise NotImplementedError("skinny_linear: the GPU path is bf16")
    K = kernels()
    x = x if x.is_contiguous() else x.contiguous()
    y = torch.empty(M, N, device=x.device, dtype=_BF16)
    S = K.skinny_splits(N, Kd)
    part = torch.empty(S * M * N, device=x.device, dtype=torch.float32) if S > 1 else None
    K.skinny_linear(x, w, b, y, part, bool(gelu))
    return y


# --------------------------------------------------------------------------------------- KV cache
class KVCache:
    """Keys and values of every layer: ``data[n_layer, 2, B, H, max_len, 64]`` bf16 (head dim 64 only)."""

    def __init__(self, cfg, batch: int, max_len: int, device=None, dtype=_BF16):
        if cfg.n_embd % cfg.n_head or cfg.n_embd // cfg.n_head != 64:
            raise NotImplementedError("KVCache: head_dim 64")
        if batch < 1 or max_len < 1:
            raise ValueError("KVCache: batch >= 1 and max_len >= 1")
        self.n_layer, self.n_head, self.batch, self.max_len = cfg.n_layer, cfg.n_head, int(batch), int(max_len)
        self.device = torch.device("cpu" if device is None else device)
        self.data = torch.zeros(cfg.n_layer, 2, batch, cfg.n_head, max_len, 64, device=self.device, dtype=dtype)
        self._part = None

    def layer(self, l: int):
        return self.data[l]

    def partials(self):
        """fp32 scratch of the decode attention: one {max, sum, 64 outputs} per (b, h, key chunk)."""
        if self._part is None:
            ch = kernels().decode_attn_chunk()
            n = self.batch * self.n_head * ((self.max_len + ch - 1) // ch) * 66
            self._part = torch.empty(n, device=self.device, dtype=torch.float32)
        return self._part


def cache_fill(qkv, cache: KVCache, layer: int, T0: int):
    """K and V of positions ``0 .. T0-1`` of a prefill c_attn output ``[B, Tpad, 3C]`` -> the layer's cache."""
    B, Tp, C3 = qkv.shape
    H = cache.n_head
    if C3 != 3 * H * 64 or B != cache.batch or not 1 <= T0 <= min(Tp, cache.max_len):
        raise ValueError(f"cache_fill: qkv {tuple(qkv.shape)} does not fit the cache / T0 = {T0}")
    if qkv.is_cuda:
        if qkv.dtype != _BF16:
            raise NotImplementedError("cache_fill: the GPU path is bf16")
        kernels().cache_fill(qkv if qkv.is_contiguous() else qkv.contiguous(), cache.layer(layer), int(T0), H)
        return
    C = C3 // 3
    for s in range(2):
        kv = qkv[:, :T0, (1 + s) * C:(2 + s) * C].reshape(B, T0, H, 64).transpose(1, 2)
        cache.data[layer, s, :, :, :T0] = kv


def decode_attention(qkv_row, cache: KVCache, layer: int, state: DecodeState):
    """One decode step of causal attention: append the new token's K and V (from its c_attn row
    ``[B, 3C]``) at the state's position ``p`` and return ``softmax(q K[0..p]^T / 8) V[0..p]`` as
    ``[B, C]``.  Fixed 128-key chunks with fp32 partials combined in chunk order: the output for a given
    ``p`` is bit-identical across runs and independent of the cache length."""
    B, C3 = qkv_row.shape
    H = cache.n_head
    if C3 != 3 * H * 64 or B != cache.batch:
        raise ValueError(f"decode_attention: qkv_row {tuple(qkv_row.shape)} does not fit the cache")
    C = C3 // 3
    scale = 1.0 / math.sqrt(64)
    if qkv_row.is_cuda:
        if qkv_row.dtype != _BF16 or cache.data.dtype != _BF16:
            raise NotImplementedError("decode_attention: the GPU path is bf16")
        out = torch.empty(B, C, device=qkv_row.device, dtype=_BF16)
        kernels().decode_attention(qkv_row if qkv_row.is_contiguous() else qkv_row.contiguous(), cache.layer(layer),
                                   state.buf, cache.partials(), out, H, scale)
        return out
    p = state.pos()
    q, k, v = (t.reshape(B, H, 64) for t in qkv_row.split(C, dim=1))
    cache.data[layer, 0, :, :, p] = k
    cache.data[layer, 1, :, :, p] = v
    Kc, Vc = cache.data[layer, 0, :, :, :p + 1].float(), cache.data[layer, 1, :, :, :p + 1].float()
    s = torch.einsum("bhd,bhtd->bht", q.float(), Kc) * scale
    return torch.einsum("bht,bhtd->bhd", torch.softmax(s, -1), Vc).reshape(B, C).to(qkv_row.dtype)


def decode_embed(tok, wte, wpe, state: DecodeState):
    """``x[b] = wte[tok[b]] + wpe[p]`` with ``p`` read from the state."""
    if wte.is_cuda:
        if wte.dtype != _BF16 or wpe.dtype != _BF16 or wte.shape[1] % 8:
            raise NotImplementedError("decode_embed: the GPU path is bf16 with C % 8 == 0")
        out = torch.empty(tok.numel(), wte.shape[1], device=wte.device, dtype=_BF16)
        kernels().decode_embed(tok, wte, wpe, state.buf, out)
        return out
    return F.embedding(tok, wte) + wpe[state.pos()].unsqueeze(0)


# --------------------------------------------------------------------------------------- sampling
def _snapshot_of(snapshot_or_state):
    return snapshot_or_state.rng if isinstance(snapshot_or_state, DecodeState) else snapshot_or_state


def sample_reference(logits, V: int, snapshot_or_state, temperature: float = 1.0, top_k=None,
                     return_info: bool = False):
    """The sampling definition in numpy, fp64, from the same Philox words as the kernel.  ``logits`` is
    ``[B, Vp]`` (any float dtype; columns ``>= V`` never participate).  Returns the ``[B]`` int64 tokens,
    and with ``return_info`` also a dict: ``threshold`` (the k-th largest value per row, ``-inf`` without
    top-k), ``ncand`` (candidates per row) and ``gap`` (best minus runner-up score per row, ``inf`` with a
    single candidate or for greedy)."""
    if logits.dim() != 2 or not 1 <= V <= logits.shape[1]:
        raise ValueError("sample_reference: logits [B, Vp] with 1 <= V <= Vp")
    if temperature < 0:
        raise ValueError("temperature must be >= 0")
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be >= 1")
    B, Vp = logits.shape
    lg = logits.detach().float().cpu().numpy().astype(np.float64)[:, :V]
    thr = np.full(B, -np.inf)
    gap = np.full(B, np.inf)
    if temperature == 0:
        tok = lg.argmax(axis=1)                       # first occurrence = lowest index
        ncand = np.full(B, V)
    else:
        if top_k is not None and top_k < V:
            thr = np.partition(lg, V - top_k, axis=1)[:, V - top_k]
        cand = lg >= thr[:, None]
        ngrp = (Vp + 3) // 4
        groups = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(ngrp)
                  + np.arange(ngrp, dtype=np.uint64)[None, :])
        w = np.stack(R._words(_snapshot_of(snapshot_or_state), 0, groups), axis=2).reshape(B, ngrp * 4)[:, :V]
        u = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        g = -np.log(-np.log(u))
        inv_temp = float(np.float32(1.0 / temperature))
        score = np.where(cand, lg * inv_temp + g, -np.inf)
        tok = score.argmax(axis=1)
        ncand = cand.sum(axis=1)
        if V > 1:
            top2 = np.partition(score, V - 2, axis=1)[:, V - 2:]
            with np.errstate(invalid="ignore"):
                gap = np.where(ncand > 1, top2[:, 1] - top2[:, 0], np.inf)
    tok = torch.from_numpy(tok.astype(np.int64))
    if return_info:
        return tok, {"threshold": thr, "ncand": ncand, "gap": gap}
    return tok


def key16_to_float(key):
    """The bf16 value of the sampler's order-preserving 16-bit key (int tensor) as float64; key 0 (no
    top-k) gives ``-inf``."""
    k = key.detach().cpu().numpy().astype(np.int64) & 0xFFFF
    bits = np.where(k & 0x8000, k & 0x7FFF, ~k & 0xFFFF).astype(np.uint32) << np.uint32(16)
    val = bits.view(np.float32).astype(np.float64)
    return np.where(k == 0, -np.inf, val)


def sample(logits, V: int, snapshot_or_state, temperature: float = 1.0, top_k=None, eos_token_id=None,
           next=None, out=None, logits_out=None, T0: int = 0, threshold_out=None):
    """Sample one token per row of the ``[B, Vp]`` bf16 logits on the device (one block per row).

    With a ``DecodeState`` the launch also does the bookkeeping of a generation step: the token goes to
    ``next[b]`` and ``out[b, T0 + step]``; a finished row emits ``eos_token_id`` and a row that emits it
    becomes finished; ``logits_out[b, step, :]`` receives the row's first ``V`` logits; then position, step
    and draw number advance.  ``threshold_out`` (int32 ``[B]``, GPU, for tests) receives the top-k threshold
    as the kernel's order-preserving 16-bit key (``key16_to_float`` decodes it).  With a plain 4-word RNG snapshot a temporary state is used.  Returns ``next``.
    CPU tensors run ``sample_reference`` (with the same bookkeeping on a ``DecodeState``)."""
    if temperature < 0:
        raise ValueError("temperature must be >= 0")
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be >= 1")
    B = logits.shape[0]
    if isinstance(snapshot_or_state, DecodeState):
        state = snapshot_or_state
    else:
        state = DecodeState(logits.device, snapshot_or_state)
    if next is None:
        next = torch.zeros(B, device=logits.device, dtype=torch.int64)
    if out is None:
        out = torch.zeros(B, T0 + 1, device=logits.device, dtype=torch.int64)
    eos = -1 if eos_token_id is None else int(eos_token_id)
    if not logits.is_cuda:
        tok = sample_reference(logits, V, state, temperature, top_k)
        step = state.step()
        if eos >= 0:
            fin = state.finished[:B].bool()
            tok = torch.where(fin, torch.full_like(tok, eos), tok)
            state.finished[:B] = (fin | (tok == eos)).int()
        next.copy_(tok)
        if T0 + step < out.shape[1]:
            out[:, T0 + step] = tok
        if logits_out is not None and step < logits_out.shape[1]:
            logits_out[:, step] = logits[:, :V].to(logits_out.dtype)
        state.advance_()
        return next
    if logits.dim() != 2 or logits.dtype != _BF16 or logits.shape[1] % 8 or not logits.is_contiguous():
        raise NotImplementedError("sample: the GPU path takes contiguous bf16 logits [B, Vp] with Vp % 8 == 0")
    if B > MAX_ROWS:
        raise NotImplementedError(f"sample: at most {MAX_ROWS} rows on the GPU (got {B})")
    greedy = temperature == 0
    inv_temp = 0.0 if greedy else float(np.float32(1.0 / temperature))
    kernels().decode_sample(logits, int(V), state.buf, next, out, logits_out, int(T0), inv_temp, greedy,
                            0 if top_k is None else int(top_k), eos, threshold_out)
    return next
