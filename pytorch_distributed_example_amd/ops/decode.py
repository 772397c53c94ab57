"""GPT-2 generation ops (bf16) over the HIP kernels of ``csrc/kernels/decode.hip``: skinny linear
(``M <= 16`` rows), KV cache with decode attention, decode embedding, and the device-side sampler with
its CPU twin.

Everything that changes from token to token -- position, output slot, RNG draw number, the rows'
"finished" flags -- lives in a small device buffer (``DecodeState``, layout in
``csrc/include/pde_decode.h``) that the kernels read and the sampler advances, so one decode step can be
captured once and replayed per token with no host work in between.  The same buffer holds one constant
position offset per row, ``off_b = len_b - max(len) <= 0``, for a batch of prompts of different lengths:
row ``b`` is at position ``pos + off_b`` and its token goes to ``out[b, T0 + off_b + step]``.

Sampling definition (``sample`` on the GPU and ``sample_reference`` in numpy compute the same thing):

* ``temperature == 0``: the lowest index attaining the row maximum over the first ``V`` columns.
* otherwise ``top_k = k`` keeps ``{v : logit_v >= k-th largest logit value of the row}`` -- ties at the
  threshold are kept, so the set can exceed ``k`` -- and the token is
  ``argmax_v(float(logit_v) * fp32(1 / temperature) + g_v)`` over that set, lowest index on ties, with the
  Gumbel noise ``g_v = -log(-log(u_v))``, ``u_v = ((w_v >> 9) + 0.5) * 2^-23`` and ``w_v`` word ``v & 3`` of
  Philox group ``b * ceil(Vp / 4) + (v >> 2)`` at site 0 of the snapshot (``ops/rng.py`` addressing).
  This is the Gumbel-max form of sampling from ``softmax(logits / temperature)``; one draw number per token.
* ``top_p = P`` in ``(0, 1)`` (``None`` and ``1.0``: off; ignored when ``temperature == 0``) comes after
  top-k.  With ``C`` the candidates after top-k (all ``V`` columns without it),
  ``z_v = float(logit_v) * fp32(1 / temperature)``, ``w_v = exp(z_v - max_C z)``, ``W = sum_C w_v`` and, for a
  bf16 value ``t``, ``M>=(t)`` the sum of ``w_v`` over the candidates with ``logit_v >= t`` (``M>(t)``: with
  ``>``), the nucleus threshold ``t_p`` is the largest logit value occurring in ``C`` with
  ``M>=(t_p) >= P * W``, and the kept set is ``{v in C : logit_v >= t_p}``: a threshold value with ties kept,
  like top-k, never empty, and ``t_p >=`` the top-k threshold, so ``t_p`` is the effective threshold.  The
  token is the same Gumbel-max over the kept set, same Philox addressing.  The kernel sums ``w_v`` as
  ``round(2^40 * expf(.))`` in 64-bit integers (order-independent; at most ``50304 * 2^-41`` of ``W`` off),
  the reference in fp64; ``p_slack`` of ``sample_reference`` says how far ``P * W`` is from the nearest
  boundary at which the two could disagree.

Logit processors (``LogitProcessors``; ``sample`` on the GPU and ``process_logits_reference`` in numpy
float32 compute the same bits).  Consider row ``b`` at generation step ``s`` (the state's step, 0 for the first
generated token), ``x_v`` the model's logit converted to fp32, ``v < V``.  The prompt of row ``b`` is
``idx[b, :len_b]`` and its generated tokens so far are what was written to ``out[b, len_b : len_b + s]``, eos
forced on a finished row included.  ``TokenCounts`` holds that history on the device::

    n_v    = number of times v occurs among the generated tokens of row b so far
    seen_v = n_v > 0 or v occurs in the prompt of row b

    1. repetition (r > 0, 1 = off):   if seen_v:  x = x * fp32(1 / r) if x > 0 else x * fp32(r)
    2. frequency f, presence p:       x = (x - fp32(f) * float(n_v)) - (fp32(p) if n_v > 0 else 0)
    3. bias (fp32 [V] or [B, V]):     x = x + bias[b, v]              (-inf bans v; +inf and NaN are rejected)
    4. min_new_tokens m (needs eos):  if s < m and v == eos:  x = -inf
    5. y_v = x rounded to the logits' dtype, round-to-nearest-even    (bf16 on the GPU)

The order is vLLM's: repetition applies to prompt and output, frequency / presence to output only.  Every fp32
operation is rounded on its own (no fused multiply-add); the two factors of step 1 are computed on the host;
step 3 is skipped without a bias (``suppress_tokens`` are a bias of ``-inf``).  The sampling definition above
then applies to ``y``, unchanged.  ``return_logits`` / ``logits_out`` keep returning the raw model logits.  A
row whose every token is banned is the caller's error: it yields some token ``< V``.

History constraints (``HistoryConstraints``; ``sample(..., history=)`` on the GPU, ``history_bans_reference`` and the
stop rule of ``sample`` on the CPU).  For row ``b`` at generation step ``s``, ``len_b`` its prompt length,
``L = len_b + s`` and ``h[0 .. L-1] = out[b, 0 : L]`` -- the prompt, then what the row generated, eos forced on
a finished row included:

1. No-repeat n-gram, ``no_repeat_ngram_size = n >= 1`` (0: off).  If ``L >= n - 1``, let
   ``P = h[L-n+1 .. L-1]`` (``n - 1`` tokens, empty for ``n = 1``).  Token ``v`` is banned iff some ``j`` with
   ``n-1 <= j <= L-1`` has ``h[j-n+1 .. j-1] == P`` and ``h[j] == v``.  The prompt counts, as in Hugging Face's
   ``NoRepeatNGramLogitsProcessor``, and so does ``j = L-1``: the matched window may overlap ``P`` itself (with
   ``n = 2``, a history ``.. a a`` bans ``a``).  ``n = 1`` bans every token of the history.
2. Banned sequences, ``bad_words_ids``: token lists of length ``m >= 1``.  ``m == 1`` is merged into the bias as
   ``-inf`` on the host, as ``suppress_tokens`` are.  For ``m > 1``: if ``L >= m-1`` and
   ``h[L-m+1 .. L-1] == seq[:m-1]``, then ``seq[m-1]`` is banned.
3. A ban sets ``x = -inf`` between steps 3 (bias) and 4 (``min_new_tokens``) of the processors above; steps 5 and
   the sampling are unchanged, ``return_logits`` stays raw.  A finished row ignores bans: it emits eos.  History
   tokens outside ``[0, V)`` ban nothing.  A row with every token banned is the caller's error, as above.
4. Stop sequences, ``stop_sequences``: token lists of length ``m >= 1``; they need ``eos_token_id``.  A row that
   was not finished emits ``tok`` at step ``s``; if ``s + 1 >= m`` and ``out[b, len_b+s-m+1 .. len_b+s] == seq``
   with ``tok`` in place, the row becomes finished.  The match lies entirely in the generated tokens: a stop
   sequence that begins in the prompt does not fire.  The sequence stays in ``out``; from the next step on the
   row emits ``eos_token_id``, exactly as after an emitted eos.  ``min_new_tokens`` concerns eos only and does
   not delay a stop.  ``stop_hit[b]`` (int32) is ``-1``, or the lowest index in list order of a sequence that
   matched when the row finished.

Beam search (``BeamConfig``; ``beam_step`` on the GPU, ``beam_step_reference`` in numpy fp64).  ``num_beams = K``,
prompts ``b = 0 .. B-1``, physical rows ``r = b * K + k``, ``R = B * K``.  Row ``r`` carries ``S[r]`` (cumulative
log-probability, fp32 on the device), ``fin[r]`` and ``len[r]`` (generated tokens, the eos that finished it
included).  It is deterministic and draws no random number.  At step ``s`` (0 = first generated token) the
candidates of group ``b`` are::

    row r live:      cand(k, v) = S[r] + (x_v - lse_r)  for every v < V,  x_v = float(logits[r, v]),
                     lse_r = logsumexp(x[:V])
    row r finished:  one candidate, cand(k, eos) = S[r]   (frozen: it keeps emitting eos, its score stands)
    step 0:          only k = 0 exists (the prompt's logits, S = 0); needs V >= K

The new beams ``j = 0 .. K-1`` are the ``K`` largest candidates in descending order, the lower flat index
``k * V + v`` first among equal scores.  Beam ``j`` from candidate ``(k, v)``: ``parent[s][b*K+j] = k``,
``tok[s][b*K+j] = v``, ``S' = cand``, ``fin' = fin[k] or v == eos``, ``len' = len[k] + (0 if fin[k] else 1)``.  Without
an eos no beam finishes.  Every step runs; finished beams are frozen, so stopping early would change nothing.  The
final ranking is by ``S / len ** length_penalty`` descending, the lower beam first on ties, and a hypothesis is
recovered by walking ``parent`` backwards from its last row.

The KV cache is never reordered for it.  ``beam_table`` is a per-row ancestor table -- which physical row holds each
position's K and V of the hypothesis living in row ``r`` -- that ``decode_attention(beam_table=)`` reads through and
the beam step rewrites into its other half (``PdeBeamTable`` in ``pde_decode.h``); the prompt's K and V are stored
once per prompt (``cache_fill(num_beams=)``).

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

STATE_WORDS = 40          # pde_decode.h
_RNG, _POS, _STEP, _FIN = 0, 4, 5, 8
MAX_ROWS = 16


def _int_list(x):
    """A list or int tensor as a list of Python ints (a host read for a device tensor)."""
    return [int(n) for n in (x.tolist() if torch.is_tensor(x) else x)]


def check_top_p(top_p, who: str = "sample"):
    """``None`` or a value in ``(0, 1]``; returns whether the nucleus stage is on (``None`` and 1.0: off)."""
    if top_p is None:
        return False
    if not 0.0 < float(top_p) <= 1.0:
        raise ValueError(f"{who}: top_p must be None or in (0, 1] (got {top_p})")
    return float(top_p) < 1.0


class DecodeState:
    """The device-side state of a generation: RNG words, position, step, and one finished flag and one position
    offset per row (int32: 8 words, ``rows`` flags, ``rows`` offsets).  With the default 16 rows it is the 40-word
    layout of ``pde_decode.h``, the only one the kernels take; a CPU state may hold more rows."""

    def __init__(self, device=None, rng_state=None, pos: int = 0, step: int = 0, row_offsets=None,
                 rows: int = MAX_ROWS):
        self.device = torch.device("cpu" if device is None else device)
        self.rows = int(rows)
        if self.rows < 1 or (self.rows != MAX_ROWS and self.device.type != "cpu"):
            raise ValueError(f"DecodeState: {MAX_ROWS} rows on the GPU, any number >= 1 on the CPU (got {rows})")
        self._off = _FIN + self.rows
        self.buf = torch.zeros(self._off + self.rows, dtype=torch.int32, device=self.device)
        self.reset(rng_state, pos, step, row_offsets)

    def reset(self, rng_state=None, pos: int = 0, step: int = 0, row_offsets=None):
        """Position / step / row offsets from the host, RNG words copied from a ``DeviceRNG`` state or
        snapshot (a device-to-device copy: no host read); the finished flags are cleared.  ``row_offsets``
        (up to ``rows`` ints ``<= 0``, default all 0) are ``len_b - max(len)`` of a ragged prompt batch: row ``b``
        is at position ``pos + row_offsets[b]``."""
        init = torch.zeros(self.buf.numel(), dtype=torch.int32)
        init[_POS], init[_STEP] = int(pos), int(step)
        if row_offsets is not None:
            offs = _int_list(row_offsets)
            if len(offs) > self.rows or any(o > 0 for o in offs):
                raise ValueError(f"row_offsets: at most {self.rows} values <= 0 (got {offs})")
            init[self._off:self._off + len(offs)] = torch.tensor(offs, dtype=torch.int32)
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
        return self.buf[_FIN:_FIN + self.rows]

    @property
    def row_offsets(self):
        return self.buf[self._off:self._off + self.rows]

    def pos(self) -> int:
        """The base position: that of the rows with offset 0 (the longest prompts)."""
        return int(self.buf[_POS].item())

    def offsets(self, B: int = None):
        """The position offsets of rows ``0 .. B-1`` (default: all) as a list (a host read)."""
        if B is not None and B > self.rows:
            raise ValueError(f"a batch of {B} rows on a decode state of {self.rows}")
        return self.row_offsets[:B].tolist()

    def row_pos(self, B: int = None):
        """The positions of rows ``0 .. B-1`` (default: all) as a list: base position plus row offset (a host read)."""
        pos = self.pos()
        return [pos + o for o in self.offsets(B)]

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


def cache_fill(qkv, cache: KVCache, layer: int, T0: int, num_beams: int = 1):
    """K and V of positions ``0 .. T0-1`` of a prefill c_attn output ``[B, Tpad, 3C]`` -> the layer's cache.  With
    ``num_beams = K > 1`` the cache holds ``B * K`` rows and prompt ``b`` goes to row ``b * K``, the one the initial
    ancestor table of a beam search (``beam_table``) points the whole group at."""
    B, Tp, C3 = qkv.shape
    H, K = cache.n_head, int(num_beams)
    if C3 != 3 * H * 64 or K < 1 or B * K != cache.batch or not 1 <= T0 <= min(Tp, cache.max_len):
        raise ValueError(f"cache_fill: qkv {tuple(qkv.shape)} does not fit the cache / T0 = {T0}")
    if qkv.is_cuda:
        if qkv.dtype != _BF16:
            raise NotImplementedError("cache_fill: the GPU path is bf16")
        qkv = qkv if qkv.is_contiguous() else qkv.contiguous()
        if K > 1:
            if B * K > MAX_ROWS:
                raise NotImplementedError(f"cache_fill: B * num_beams <= {MAX_ROWS} rows on the GPU (got {B * K})")
            kernels().cache_fill_beam(qkv, cache.layer(layer), int(T0), H, K)
        else:
            kernels().cache_fill(qkv, cache.layer(layer), int(T0), H)
        return
    C = C3 // 3
    for s in range(2):
        kv = qkv[:, :T0, (1 + s) * C:(2 + s) * C].reshape(B, T0, H, 64).transpose(1, 2)
        cache.data[layer, s, ::K, :, :T0] = kv


def decode_attention(qkv_row, cache: KVCache, layer: int, state: DecodeState, beam_table=None):
    """One decode step of causal attention: append the new token's K and V (from its c_attn row
    ``[B, 3C]``) at the state's position ``p`` and return ``softmax(q K[0..p]^T / 8) V[0..p]`` as
    ``[B, C]``.  Fixed 128-key chunks with fp32 partials combined in chunk order: the output for a given
    ``p`` is bit-identical across runs and independent of the cache length.  ``p`` is per row, ``p_b`` = the
    state's position plus row ``b``'s offset, and a row's output depends on its own ``p_b`` only: it is
    bit-identical to a call in which every row is at ``p_b``.

    ``beam_table`` (uint8 ``[2, 16, stride >= max_len]``, see ``beam_table()``) is a beam search's ancestor table:
    key and value ``j < p_b`` of row ``b`` are read from cache row ``table[step & 1, b, j]``, with ``step`` the state's;
    position ``p_b`` is still appended to row ``b`` itself.  The arithmetic is the same, so the output is
    bit-identical to the call without a table on a cache gathered through it."""
    B, C3 = qkv_row.shape
    H = cache.n_head
    if C3 != 3 * H * 64 or B != cache.batch:
        raise ValueError(f"decode_attention: qkv_row {tuple(qkv_row.shape)} does not fit the cache")
    C = C3 // 3
    scale = 1.0 / math.sqrt(64)
    if qkv_row.is_cuda:
        if qkv_row.dtype != _BF16 or cache.data.dtype != _BF16:
            raise NotImplementedError("decode_attention: the GPU path is bf16")
        if B > MAX_ROWS:
            raise NotImplementedError(f"decode_attention: at most {MAX_ROWS} rows on the GPU (got {B})")
        out = torch.empty(B, C, device=qkv_row.device, dtype=_BF16)
        qkv_row = qkv_row if qkv_row.is_contiguous() else qkv_row.contiguous()
        if beam_table is None:
            kernels().decode_attention(qkv_row, cache.layer(layer), state.buf, cache.partials(), out, H, scale)
        else:
            kernels().decode_attention_beam(qkv_row, cache.layer(layer), state.buf, cache.partials(), out, H, scale,
                                            beam_table)
        return out
    q, k, v = (t.reshape(B, H, 64) for t in qkv_row.split(C, dim=1))
    rows = []
    anc = None if beam_table is None else beam_table[state.step() & 1].long()
    for b, p in enumerate(state.row_pos(B)):
        cache.data[layer, 0, b, :, p] = k[b]
        cache.data[layer, 1, b, :, p] = v[b]
        if anc is None:
            Kc, Vc = cache.data[layer, 0, b, :, :p + 1].float(), cache.data[layer, 1, b, :, :p + 1].float()
        else:       # positions < p through the table ([p, H, 64] -> [H, p, 64]), position p from the row itself
            src, t = torch.cat([anc[b, :p], torch.tensor([b])]), torch.arange(p + 1)
            Kc, Vc = (cache.data[layer, s][src, :, t].transpose(0, 1).float() for s in (0, 1))
        s = torch.einsum("hd,htd->ht", q[b].float(), Kc) * scale
        rows.append(torch.einsum("ht,htd->hd", torch.softmax(s, -1), Vc).reshape(C))
    return torch.stack(rows).to(qkv_row.dtype)


def decode_embed(tok, wte, wpe, state: DecodeState):
    """``x[b] = wte[tok[b]] + wpe[p_b]`` with ``p_b`` (position plus row offset) read from the state."""
    if wte.is_cuda:
        if wte.dtype != _BF16 or wpe.dtype != _BF16 or wte.shape[1] % 8:
            raise NotImplementedError("decode_embed: the GPU path is bf16 with C % 8 == 0")
        if tok.numel() > MAX_ROWS:
            raise NotImplementedError(f"decode_embed: at most {MAX_ROWS} rows on the GPU (got {tok.numel()})")
        out = torch.empty(tok.numel(), wte.shape[1], device=wte.device, dtype=_BF16)
        kernels().decode_embed(tok, wte, wpe, state.buf, out)
        return out
    return F.embedding(tok, wte) + wpe[torch.tensor(state.row_pos(tok.numel()), dtype=torch.int64)]


# --------------------------------------------------------------------------------------- sampling
def _snapshot_of(snapshot_or_state):
    return snapshot_or_state.rng if isinstance(snapshot_or_state, DecodeState) else snapshot_or_state


def _nucleus(lg, cand, inv_temp, ps):
    """The nucleus thresholds of the rows of ``lg`` (fp64 ``[B, V]``) over the candidates ``cand`` for each
    mass ``P`` in ``ps``: a list of ``(t_p, M>(t_p) / W, M>=(t_p) / W)``, each ``[B]``.  ``W`` is the last value
    of the same running sum the masses are read from, so ``P = 1`` always finds the smallest candidate."""
    B, V = lg.shape
    z = np.where(cand, lg * inv_temp, -np.inf)
    w = np.exp(z - z.max(axis=1, keepdims=True))              # 0 outside the candidates
    order = np.argsort(-lg, axis=1, kind="stable")
    sv = np.take_along_axis(lg, order, axis=1)
    sc = np.take_along_axis(cand, order, axis=1)
    cw = np.cumsum(np.take_along_axis(w, order, axis=1), axis=1)
    W = cw[:, -1]
    end = np.ones((B, V), dtype=bool)                         # last column of a run of equal values
    end[:, :-1] = sv[:, :-1] != sv[:, 1:]
    rows = np.arange(B)
    res = []
    for P in ps:
        ok = end & sc & (cw >= (P * W)[:, None])
        i = ok.argmax(axis=1)                                 # first in descending order = largest value
        assert ok[rows, i].all()
        t = sv[rows, i]
        above = np.where(sv > t[:, None], cw, 0.0).max(axis=1)    # cw is non-decreasing: M>(t)
        res.append((t, above / W, cw[rows, i] / W))
    return res


def sample_reference(logits, V: int, snapshot_or_state, temperature: float = 1.0, top_k=None,
                     return_info: bool = False, top_p=None, eps: float = 1e-4, _threshold=None):
    """The sampling definition in numpy, fp64, from the same Philox words as the kernel.  ``logits`` is
    ``[B, Vp]`` (any float dtype; columns ``>= V`` never participate).  Returns the ``[B]`` int64 tokens,
    and with ``return_info`` also a dict: ``threshold`` (the effective threshold per row: the k-th largest
    value, raised to the nucleus threshold with ``top_p``; ``-inf`` with neither), ``ncand`` (candidates per
    row) and ``gap`` (best minus runner-up score per row, ``inf`` with a single candidate or for greedy).

    With ``top_p`` on, the dict also holds ``threshold_p`` (``t_p`` of the module docstring), ``p_slack``
    (``min(top_p * W - M>(t_p), M>=(t_p) - top_p * W) / W``: how far the target mass is from the nearest
    boundary between two thresholds) and ``threshold_p_bracket``, the pair ``(t_p at top_p + eps, t_p at
    top_p - eps)`` with ``top_p +- eps`` clamped into ``(0, 1]``: the thresholds an implementation whose
    mass sums are off by less than ``eps * W`` can arrive at lie between the two.

    ``_threshold`` (``[B]`` values) replaces the computed effective threshold: the token for a threshold
    chosen elsewhere."""
    if logits.dim() != 2 or not 1 <= V <= logits.shape[1]:
        raise ValueError("sample_reference: logits [B, Vp] with 1 <= V <= Vp")
    if temperature < 0:
        raise ValueError("temperature must be >= 0")
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be >= 1")
    nucleus = check_top_p(top_p, "sample_reference")
    B, Vp = logits.shape
    lg = logits.detach().float().cpu().numpy().astype(np.float64)[:, :V]
    thr = np.full(B, -np.inf)
    gap = np.full(B, np.inf)
    extra = {}
    if temperature == 0:
        tok = lg.argmax(axis=1)                       # first occurrence = lowest index
        ncand = np.full(B, V)
    else:
        inv_temp = float(np.float32(1.0 / temperature))
        if _threshold is not None:
            thr = np.asarray(_threshold, dtype=np.float64).reshape(B)
        else:
            if top_k is not None and top_k < V:
                thr = np.partition(lg, V - top_k, axis=1)[:, V - top_k]
            if nucleus:
                P = float(top_p)
                tiny = float(np.finfo(np.float64).tiny)
                at, hi, lo = _nucleus(lg, lg >= thr[:, None], inv_temp,
                                      [P, min(P + eps, 1.0), max(P - eps, tiny)])
                thr = at[0]
                extra = {"threshold_p": at[0], "p_slack": np.minimum(P - at[1], at[2] - P),
                         "threshold_p_bracket": (hi[0], lo[0])}
        cand = lg >= thr[:, None]
        ngrp = (Vp + 3) // 4
        groups = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(ngrp)
                  + np.arange(ngrp, dtype=np.uint64)[None, :])
        w = np.stack(R._words(_snapshot_of(snapshot_or_state), 0, groups), axis=2).reshape(B, ngrp * 4)[:, :V]
        u = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        g = -np.log(-np.log(u))
        score = np.where(cand, lg * inv_temp + g, -np.inf)
        tok = score.argmax(axis=1)
        ncand = cand.sum(axis=1)
        if V > 1:
            top2 = np.partition(score, V - 2, axis=1)[:, V - 2:]
            with np.errstate(invalid="ignore"):
                gap = np.where(ncand > 1, top2[:, 1] - top2[:, 0], np.inf)
    tok = torch.from_numpy(tok.astype(np.int64))
    if return_info:
        return tok, {"threshold": thr, "ncand": ncand, "gap": gap, **extra}
    return tok


def key16_to_float(key):
    """The bf16 value of the sampler's order-preserving 16-bit key (int tensor) as float64; key 0 (no
    top-k) gives ``-inf``."""
    k = key.detach().cpu().numpy().astype(np.int64) & 0xFFFF
    bits = np.where(k & 0x8000, k & 0x7FFF, ~k & 0xFFFF).astype(np.uint32) << np.uint32(16)
    val = bits.view(np.float32).astype(np.float64)
    return np.where(k == 0, -np.inf, val)


# --------------------------------------------------------------------------------------- logit processors
class TokenCounts:
    """The history the logit processors depend on: int32 ``[B, Vp]`` (layout in ``pde_decode.h``).  Bit 30 of
    word ``(b, v)`` says that ``v`` occurs in the prompt of row ``b``; bits 0..29 count how often row ``b`` has
    generated ``v``.  The sampler reads the buffer and adds the token it emits, so a captured decode step
    follows the history on every replay."""

    PROMPT = 1 << 30
    COUNT = PROMPT - 1

    def __init__(self, B: int, Vp: int, device=None):
        if B < 1 or Vp < 1:
            raise ValueError("TokenCounts: B >= 1 and Vp >= 1")
        self.device = torch.device("cpu" if device is None else device)
        self.buf = torch.zeros(int(B), int(Vp), dtype=torch.int32, device=self.device)

    def add_prompt(self, idx, state_or_lens=None, T0=None):
        """Set the prompt flag of every token of ``idx[b, :len_b]``.  ``state_or_lens`` is a ``DecodeState``
        (``len_b = T0 + row offset``, read on the device; ``T0`` defaults to the width of ``idx``), a list of
        ``B`` lengths, or ``None`` (every column).  Columns past ``len_b`` are never counted, whatever they
        hold.  To be called before the first token is generated: the counts are zero then, which is what
        lets the kernel store the flag word without an atomic."""
        B, Vp = self.buf.shape
        if idx.dim() != 2 or idx.shape[0] != B or idx.shape[1] < 1:
            raise ValueError(f"add_prompt: idx must be [{B}, width >= 1] (got {tuple(idx.shape)})")
        width = idx.shape[1]
        if isinstance(state_or_lens, DecodeState):
            state, T0 = state_or_lens, width if T0 is None else int(T0)
        else:
            lens = [width] * B if state_or_lens is None else _int_list(state_or_lens)
            if len(lens) != B or min(lens) < 0 or max(lens) > width:
                raise ValueError(f"add_prompt: {B} lengths in 0 .. {width} (got {lens})")
            T0 = max(lens)
            state = None
        if not 0 <= T0 <= width:
            raise ValueError(f"add_prompt: 0 <= T0 <= {width} (got {T0})")
        if self.buf.is_cuda:
            if B > MAX_ROWS:
                raise NotImplementedError(f"add_prompt: at most {MAX_ROWS} rows on the GPU (got {B})")
            if state is None:
                state = DecodeState(self.device, row_offsets=[n - T0 for n in lens])
            idx = idx.to(self.device, torch.int64)
            kernels().decode_count_prompt(idx if idx.is_contiguous() else idx.contiguous(), state.buf, self.buf, T0)
            return self
        if state is not None:
            lens = [min(max(T0 + o, 0), width) for o in state.offsets(B)]
        for b, n in enumerate(lens):
            tok = idx[b, :n].long().cpu()
            tok = tok[(tok >= 0) & (tok < Vp)]
            self.buf[b, tok] |= self.PROMPT
        return self

    def add_(self, tok):
        """What the sampler does after choosing: one more occurrence of ``tok[b]`` in row ``b`` (CPU ops)."""
        rows = torch.arange(self.buf.shape[0], device=self.buf.device)
        self.buf[rows, tok.to(self.buf.device).long()] += 1
        return self

    def seen(self):
        """bool ``[B, Vp]``: the token occurs in the row's prompt or among its generated tokens."""
        return self.buf != 0

    def generated(self):
        """int32 ``[B, Vp]``: how often the row has generated the token."""
        return self.buf & self.COUNT


def _finite(x, name):
    x = float(x)
    if not math.isfinite(x):
        raise ValueError(f"LogitProcessors: {name} must be finite (got {x})")
    return x


def _token_id(t, what, exact=True):
    """``t`` as a token id, or ``ValueError`` in the name of ``what``.  ``exact`` (the history constraints) takes
    Python and numpy integers in ``[0, 2^31)`` and no bool; otherwise (the logit processors) whatever equals an
    integer ``>= 0``."""
    if exact:
        ok = not isinstance(t, bool) and isinstance(t, (int, np.integer)) and 0 <= t < 1 << 31
    else:
        ok = int(t) == t and t >= 0
    if not ok:
        raise ValueError(f"{what} must be token ids >= 0 (got {t!r})")
    return int(t)


class LogitProcessors:
    """Penalties, logit bias and ``min_new_tokens`` of a generation, validated on the host (``ValueError``).
    The definition is in the module docstring.  ``logit_bias`` is an fp32 tensor ``[V]`` or ``[B, V]`` on the
    logits' device (``-inf`` bans a token; NaN and ``+inf`` are rejected); ``suppress_tokens`` are merged into it
    as ``-inf``.  ``active`` is False when every setting is neutral: the sampler then runs as without processors."""

    def __init__(self, repetition_penalty: float = 1.0, frequency_penalty: float = 0.0, presence_penalty: float = 0.0,
                 logit_bias=None, suppress_tokens=None, min_new_tokens: int = 0, eos_token_id=None):
        self.repetition_penalty = _finite(repetition_penalty, "repetition_penalty")
        if self.repetition_penalty <= 0:
            raise ValueError(f"LogitProcessors: repetition_penalty must be > 0 (got {repetition_penalty})")
        self.frequency_penalty = _finite(frequency_penalty, "frequency_penalty")
        self.presence_penalty = _finite(presence_penalty, "presence_penalty")
        # what the kernel is given: fp32(r), fp32(1 / r), fp32(f), fp32(p)
        self.rep, self.inv_rep = np.float32(self.repetition_penalty), np.float32(1.0 / self.repetition_penalty)
        self.freq, self.pres = np.float32(self.frequency_penalty), np.float32(self.presence_penalty)
        if not (np.isfinite(self.rep) and np.isfinite(self.inv_rep) and self.rep > 0 and self.inv_rep > 0
                and np.isfinite(self.freq) and np.isfinite(self.pres)):
            raise ValueError("LogitProcessors: the penalties must be finite (and 1 / r > 0) in fp32")
        if logit_bias is not None:
            if not torch.is_tensor(logit_bias) or logit_bias.dtype != torch.float32 or logit_bias.dim() not in (1, 2):
                raise ValueError("LogitProcessors: logit_bias must be an fp32 tensor [V] or [B, V]")
            if bool((torch.isnan(logit_bias) | (logit_bias == math.inf)).any()):
                raise ValueError("LogitProcessors: logit_bias holds NaN or +inf")
        self.logit_bias = logit_bias
        if suppress_tokens is None:
            self.suppress_tokens = []
        else:
            toks = suppress_tokens.tolist() if torch.is_tensor(suppress_tokens) else suppress_tokens
            self.suppress_tokens = sorted({_token_id(t, "LogitProcessors: suppress_tokens", False) for t in toks})
        if int(min_new_tokens) != min_new_tokens or min_new_tokens < 0:
            raise ValueError(f"LogitProcessors: min_new_tokens must be an integer >= 0 (got {min_new_tokens})")
        self.min_new_tokens = int(min_new_tokens)
        self.eos_token_id = None if eos_token_id is None else _token_id(eos_token_id, "LogitProcessors: eos_token_id",
                                                                        False)
        if self.min_new_tokens > 0 and self.eos_token_id is None:
            raise ValueError("LogitProcessors: min_new_tokens > 0 needs eos_token_id")

    @property
    def active(self) -> bool:
        return (self.repetition_penalty != 1.0 or self.frequency_penalty != 0.0 or self.presence_penalty != 0.0
                or self.logit_bias is not None or bool(self.suppress_tokens) or self.min_new_tokens > 0)

    def check(self, B: int, V: int, device=None):
        """The checks that need the batch and the vocabulary: bias shape and device, token ids ``< V``."""
        lb = self.logit_bias
        if lb is not None:
            if tuple(lb.shape) not in ((V,), (B, V)):
                raise ValueError(f"LogitProcessors: logit_bias must be [{V}] or [{B}, {V}] (got {tuple(lb.shape)})")
            if device is not None and lb.device.type != torch.device(device).type:
                raise ValueError(f"LogitProcessors: logit_bias is on {lb.device}, the logits are on {device}")
        if self.suppress_tokens and self.suppress_tokens[-1] >= V:
            raise ValueError(f"LogitProcessors: suppress_tokens outside [0, {V}) (got {self.suppress_tokens})")
        if self.eos_token_id is not None and self.eos_token_id >= V:
            raise ValueError(f"LogitProcessors: eos_token_id outside [0, {V}) (got {self.eos_token_id})")
        return self

    def bias(self, B: int, V: int, Vp=None, device=None):
        """The merged bias -- ``logit_bias`` with ``-inf`` at ``suppress_tokens`` -- as fp32 ``[1 or B, Vp]`` with
        zeros in the pad columns (``Vp`` defaults to ``V``), or ``None`` without either.  The kernel reads it with
        aligned 16-byte loads; a generation prepares it once."""
        self.check(B, V, device)
        if self.logit_bias is None and not self.suppress_tokens:
            return None
        Vp = V if Vp is None else int(Vp)
        dev = torch.device("cpu" if device is None else device)
        rows = B if (self.logit_bias is not None and self.logit_bias.dim() == 2) else 1
        buf = torch.zeros(rows, Vp, dtype=torch.float32, device=dev)
        if self.logit_bias is not None:
            buf[:, :V] = self.logit_bias.to(dev).reshape(rows, V)
        if self.suppress_tokens:
            buf[:, torch.tensor(self.suppress_tokens, dtype=torch.int64, device=dev)] = -math.inf
        return buf


def process_logits_reference(logits, V: int, counts, processors: LogitProcessors, step: int, _bias=None):
    """The processors' definition (module docstring) in numpy float32, one rounded operation per line.
    ``logits`` is ``[B, Vp]`` of any float dtype, ``counts`` a ``TokenCounts`` or its int32 ``[B, Vp]`` buffer,
    ``step`` the generation step.  Returns ``[B, Vp]`` in the logits' dtype on the CPU: the columns ``< V``
    processed, the pad columns as they were."""
    if logits.dim() != 2 or not 1 <= V <= logits.shape[1]:
        raise ValueError("process_logits_reference: logits [B, Vp] with 1 <= V <= Vp")
    B = logits.shape[0]
    pr = processors
    buf = counts.buf if isinstance(counts, TokenCounts) else counts
    if tuple(buf.shape) != tuple(logits.shape) or buf.dtype != torch.int32:
        raise ValueError(f"process_logits_reference: counts must be int32 {tuple(logits.shape)}")
    bias = pr.bias(B, V) if _bias is None else _bias
    c = buf.detach().cpu().numpy()[:, :V]
    n = c & np.int32(TokenCounts.COUNT)
    nf = n.astype(np.float32)
    x = logits.detach().float().cpu().numpy()[:, :V].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(c != 0, np.where(x > 0, x * pr.inv_rep, x * pr.rep), x)
        fn = pr.freq * nf
        x = x - fn
        x = x - np.where(n > 0, pr.pres, np.float32(0))
        if bias is not None:
            x = x + bias.detach().cpu().numpy()[:, :V]
    if int(step) < pr.min_new_tokens:
        x[:, pr.eos_token_id] = -np.inf
    assert x.dtype == np.float32
    y = logits.detach().cpu().clone()
    y[:, :V] = torch.from_numpy(np.ascontiguousarray(x)).to(logits.dtype)
    return y


# --------------------------------------------------------------------------------------- history constraints
def _token_lists(seqs, name, max_len, max_seqs):
    if seqs is None:
        return []
    if torch.is_tensor(seqs):
        seqs = seqs.tolist()
    res = []
    for seq in seqs:
        seq = seq.tolist() if torch.is_tensor(seq) else seq
        if not isinstance(seq, (list, tuple)) or len(seq) == 0:
            raise ValueError(f"HistoryConstraints: {name} must be non-empty lists of token ids (got {seq!r})")
        if len(seq) > max_len:
            raise ValueError(f"HistoryConstraints: a sequence of {name} holds at most {max_len} tokens "
                             f"(got {len(seq)})")
        res.append([_token_id(t, f"HistoryConstraints: {name}") for t in seq])
    if len(res) > max_seqs:
        raise ValueError(f"HistoryConstraints: at most {max_seqs} sequences in {name} (got {len(res)})")
    return res


def _pack_table(seqs):
    """``[count + 1 offsets][tokens]`` int32 (PdeSampleHist in ``pde_decode.h``)"""
    offs = [0]
    for seq in seqs:
        offs.append(offs[-1] + len(seq))
    return torch.tensor(offs + [t for seq in seqs for t in seq], dtype=torch.int32)


class HistoryConstraints:
    """No-repeat n-gram, banned sequences and stop sequences of a generation, validated on the host
    (``ValueError``: non-integers, negative ids, empty sequences, stop sequences without ``eos_token_id``, limits
    exceeded; ids ``>= V`` in ``check``).  The definition is in the module docstring.

    Limits: ``no_repeat_ngram_size <= 8``; a sequence holds at most 16 tokens; ``bad_words_ids`` holds at most 256
    sequences of two or more tokens (single tokens are merged into the bias and not limited), ``stop_sequences``
    at most 256.  ``active`` is False when nothing is set: the sampler then runs as without constraints."""

    MAX_NGRAM, MAX_SEQ_LEN, MAX_SEQS = 8, 16, 256

    def __init__(self, no_repeat_ngram_size: int = 0, bad_words_ids=None, stop_sequences=None, eos_token_id=None):
        n = no_repeat_ngram_size
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= self.MAX_NGRAM:
            raise ValueError(f"HistoryConstraints: no_repeat_ngram_size must be an integer in 0 .. {self.MAX_NGRAM} "
                             f"(got {n!r})")
        self.no_repeat_ngram_size = int(n)
        bad = _token_lists(bad_words_ids, "bad_words_ids", self.MAX_SEQ_LEN, 1 << 30)
        self.bad_tokens = sorted({seq[0] for seq in bad if len(seq) == 1})      # merged into the bias
        self.bad_words = [seq for seq in bad if len(seq) > 1]
        if len(self.bad_words) > self.MAX_SEQS:
            raise ValueError(f"HistoryConstraints: at most {self.MAX_SEQS} sequences of two or more tokens in "
                             f"bad_words_ids (got {len(self.bad_words)})")
        self.stop_sequences = _token_lists(stop_sequences, "stop_sequences", self.MAX_SEQ_LEN, self.MAX_SEQS)
        e = eos_token_id
        if e is not None and (isinstance(e, bool) or not isinstance(e, (int, np.integer)) or e < 0):
            raise ValueError(f"HistoryConstraints: eos_token_id must be a token id >= 0 (got {e!r})")
        self.eos_token_id = None if e is None else int(e)
        if self.stop_sequences and self.eos_token_id is None:
            raise ValueError("HistoryConstraints: stop_sequences need eos_token_id")
        self._tables, self._checked = {}, set()

    @property
    def active(self) -> bool:
        return (self.no_repeat_ngram_size > 0 or bool(self.bad_words) or bool(self.bad_tokens)
                or bool(self.stop_sequences))

    def check(self, V: int):
        """The check that needs the vocabulary: token ids ``< V``."""
        if V in self._checked:
            return self
        for name, seqs in (("bad_words_ids", self.bad_words + [self.bad_tokens]),
                           ("stop_sequences", self.stop_sequences)):
            if any(t >= V for seq in seqs for t in seq):
                raise ValueError(f"HistoryConstraints: {name} outside [0, {V})")
        if self.eos_token_id is not None and self.eos_token_id >= V:
            raise ValueError(f"HistoryConstraints: eos_token_id outside [0, {V}) (got {self.eos_token_id})")
        self._checked.add(V)
        return self

    def tables(self, device=None):
        """``(banned, stop)``: the packed int32 sequence tables on ``device`` (``None`` for an empty one), made
        once per device."""
        dev = torch.device("cpu" if device is None else device)
        if dev not in self._tables:
            self._tables[dev] = tuple(_pack_table(s).to(dev) if s else None
                                      for s in (self.bad_words, self.stop_sequences))
        return self._tables[dev]

    def merge_bias(self, bias, V: int, Vp=None, device=None):
        """``bias`` (the processors' padded fp32 ``[1 or B, Vp]``, or ``None``) with ``-inf`` at the single-token
        ``bad_words_ids``: a new tensor, or ``bias`` itself without any."""
        if not self.bad_tokens:
            return bias
        self.check(V)
        if bias is None:
            bias = torch.zeros(1, V if Vp is None else int(Vp), dtype=torch.float32,
                               device=torch.device("cpu" if device is None else device))
        else:
            bias = bias.clone()
        bias[:, torch.tensor(self.bad_tokens, dtype=torch.int64, device=bias.device)] = -math.inf
        return bias


def history_bans_reference(out, lengths, V: int, history: HistoryConstraints):
    """Rules 1 and 2 of the history constraints (module docstring) in numpy: ``out`` is ``[B, >= max L]`` int64,
    ``lengths`` the ``B`` history lengths ``L = len_b + step``.  Returns bool ``[B, V]``: token ``v`` of row ``b`` is
    banned.  Single-token ``bad_words_ids`` are not here: they are part of the bias."""
    hs = out.detach().cpu().numpy()
    B = hs.shape[0]
    n = history.no_repeat_ngram_size
    ban = np.zeros((B, V), dtype=bool)
    for b in range(B):
        L = int(lengths[b])
        if not 0 <= L <= hs.shape[1]:
            raise ValueError(f"history_bans_reference: row {b} has length {L}, out holds {hs.shape[1]} columns")
        h = hs[b, :L]
        if n >= 1 and L >= n - 1:
            P = h[L - n + 1:L]
            for j in range(n - 1, L):
                if np.array_equal(h[j - n + 1:j], P) and 0 <= h[j] < V:
                    ban[b, h[j]] = True
        for seq in history.bad_words:
            m = len(seq)
            if L >= m - 1 and np.array_equal(h[L - m + 1:L], np.asarray(seq[:-1], dtype=hs.dtype)) and seq[-1] < V:
                ban[b, seq[-1]] = True
    return torch.from_numpy(ban)


class SamplerConfig:
    """The sampling settings of a generation -- ``temperature``, ``top_k``, ``top_p``, ``eos_token_id``, ``processors``
    (a ``LogitProcessors``) and ``history`` (a ``HistoryConstraints``) -- validated once (``ValueError``): the ranges,
    and that ``eos_token_id`` is the one ``min_new_tokens`` and the stop sequences were given; without one theirs is
    used.  Processors and constraints whose ``active`` is False become ``None``, except that constraints keep neutral
    processors beside them (the history kernel sits on the processors' prologue), as does ``keep_neutral``.

    Derived: ``greedy``, ``inv_temp`` (``fp32(1 / temperature)``) and ``nucleus`` (``top_p`` does something)."""

    def __init__(self, temperature: float = 1.0, top_k=None, top_p=None, eos_token_id=None, processors=None,
                 history=None, who: str = "sample", keep_neutral: bool = False):
        if temperature < 0:
            raise ValueError(f"{who}: temperature must be >= 0")
        if top_k is not None and top_k < 1:
            raise ValueError(f"{who}: top_k must be >= 1")
        self.nucleus = check_top_p(top_p, who)
        self.temperature, self.top_k, self.top_p = float(temperature), top_k, top_p
        self.greedy = temperature == 0
        self.inv_temp = 0.0 if self.greedy else float(np.float32(1.0 / temperature))
        eos = eos_token_id
        history = history if history is not None and history.active else None
        if history is not None:
            if eos is None:
                eos = history.eos_token_id
            elif history.stop_sequences and int(eos) != history.eos_token_id:
                raise ValueError(f"{who}: eos_token_id differs from the constraints' eos_token_id")
            if processors is None:
                processors = LogitProcessors(eos_token_id=eos)
        elif processors is not None and not (processors.active or keep_neutral):
            processors = None
        if processors is not None:
            if eos is None:
                eos = processors.eos_token_id
            elif processors.min_new_tokens > 0 and int(eos) != processors.eos_token_id:
                raise ValueError(f"{who}: eos_token_id differs from the processors' eos_token_id")
        self.eos_token_id = None if eos is None else int(eos)
        self.processors, self.history = processors, history
        # what the launch is given
        self._core = (self.inv_temp, self.greedy, 0 if top_k is None else int(top_k), -1 if eos is None else int(eos))
        self._top_p = float(top_p) if self.nucleus else 0.0
        self._proc = self._hist = None
        if processors is not None:
            self._proc = dict(rep=float(processors.rep), inv_rep=float(processors.inv_rep), freq=float(processors.freq),
                              pres=float(processors.pres), min_new=processors.min_new_tokens)
        if history is not None:
            self._hist = dict(ngram=history.no_repeat_ngram_size, n_ban=len(history.bad_words),
                              n_stop=len(history.stop_sequences))

    def check(self, B: int, V: int, device=None):
        """The checks that need the batch and the vocabulary: the members' own, and ``eos_token_id < V``."""
        if self.eos_token_id is not None and not 0 <= self.eos_token_id < V:
            raise ValueError("eos_token_id must be a token of the vocabulary")
        if self.processors is not None:
            self.processors.check(B, V, device)
        if self.history is not None:
            self.history.check(V)
        return self

    def bias(self, B: int, V: int, Vp: int, device=None):
        """The merged bias of processors and constraints, fp32 ``[1 or B, Vp]``, or ``None`` without processors or
        without anything to add."""
        if self.processors is None:
            return None
        bias = self.processors.bias(B, V, Vp, device)
        return bias if self.history is None else self.history.merge_bias(bias, V, Vp, device)


def _sample_cpu(cfg, logits, V, state, next, out, logits_out, T0, counts, bias, processed_out, stop_hit):
    """The CPU twin of the sampler launch: processors, bans, the choice, the eos and stop rules and the bookkeeping of
    a generation step on a CPU ``DecodeState``, in the kernel's order."""
    B = logits.shape[0]
    eos, hist = cfg._core[3], cfg.history
    step = state.step()
    offs = state.offsets(B)
    was_fin = state.finished[:B].bool() if eos >= 0 else torch.zeros(B, dtype=torch.bool)
    y = logits
    if cfg.processors is not None:
        y = process_logits_reference(logits, V, counts, cfg.processors, step, _bias=bias)
        if hist is not None:             # a finished row ignores bans: it emits eos
            ban = history_bans_reference(out, [T0 + off + step for off in offs], V, hist)
            y[:, :V][ban & ~was_fin[:, None]] = -math.inf
        if processed_out is not None:
            processed_out.copy_(y)
    tok = sample_reference(y, V, state, cfg.temperature, cfg.top_k, top_p=cfg.top_p)
    if eos >= 0:
        tok = torch.where(was_fin, torch.full_like(tok, eos), tok)
        state.finished[:B] = (was_fin | (tok == eos)).int()
    if hist is not None and hist.stop_sequences:
        for b, off in enumerate(offs):
            if was_fin[b]:
                continue
            gen = out[b, T0 + off:T0 + off + step].tolist() + [int(tok[b])]
            for q, seq in enumerate(hist.stop_sequences):
                if len(gen) >= len(seq) and gen[len(gen) - len(seq):] == seq:
                    state.finished[b] = 1
                    stop_hit[b] = q
                    break
    next.copy_(tok)
    for b, off in enumerate(offs):
        if 0 <= T0 + off + step < out.shape[1]:
            out[b, T0 + off + step] = tok[b]
    if logits_out is not None and step < logits_out.shape[1]:
        logits_out[:, step] = logits[:, :V].to(logits_out.dtype)
    if cfg.processors is not None:
        counts.add_(tok)
    state.advance_()
    return next


def sample(logits, V: int, snapshot_or_state, temperature: float = 1.0, top_k=None, eos_token_id=None,
           next=None, out=None, logits_out=None, T0: int = 0, threshold_out=None, top_p=None,
           processors=None, counts=None, processed_out=None, _force_proc=False, _bias=None, history=None,
           stop_hit=None, config=None):
    """Sample one token per row of the ``[B, Vp]`` bf16 logits on the device (one block per row).

    With a ``DecodeState`` the launch also does the bookkeeping of a generation step: the token goes to
    ``next[b]`` and ``out[b, T0 + off_b + step]`` (``off_b``: the state's row offset, 0 for a batch of one
    prompt length); a finished row emits ``eos_token_id`` and a row that emits it
    becomes finished; ``logits_out[b, step, :]`` receives the row's first ``V`` logits; then position, step
    and draw number advance.  ``threshold_out`` (int32 ``[B]``, GPU, for tests) receives the effective
    threshold (top-k, raised by ``top_p``) as the kernel's order-preserving 16-bit key (``key16_to_float``
    decodes it).  ``top_p`` of ``None`` or 1.0 runs the sampler without the nucleus stage.  With a plain
    4-word RNG snapshot a temporary state is used.  Returns ``next``.

    ``processors`` (a ``LogitProcessors``) with ``counts`` (the ``TokenCounts`` of the generation) applies the
    logit processors of the module docstring at the state's step before sampling, and adds the emitted token
    (the eos forced on a finished row included) to ``counts``.  ``processed_out`` (``[B, Vp]`` in the logits'
    dtype) receives the processed logits ``y``; on the GPU it is the kernel's workspace and all ``Vp`` columns are
    written.  ``logits_out`` receives the raw logits all the same.  Processors whose ``active`` is False run the
    sampler exactly as without them.  Their ``eos_token_id`` stands in for a missing ``eos_token_id`` here.
    CPU tensors run ``process_logits_reference`` and ``sample_reference`` (with the same bookkeeping on a
    ``DecodeState``).

    ``history`` (a ``HistoryConstraints``) applies the history constraints of the module docstring.  The history
    of row ``b`` is ``out[b, : T0 + off_b + step]``, so ``out`` is needed and holds the prompts; stop sequences
    need ``stop_hit`` (int32 ``[B]`` on the logits' device, ``-1`` in rows that have not stopped) and an eos.  The
    constraints run on top of the processors' kernel: without ``processors`` neutral ones are used, and without
    ``counts`` a scratch one.  Constraints whose ``active`` is False change nothing.  CPU tensors run
    ``history_bans_reference`` and the stop rule with the same bookkeeping.

    ``config`` (a ``SamplerConfig``) stands for ``temperature``, ``top_k``, ``top_p``, ``eos_token_id``, ``processors``
    and ``history``, which are then ignored, and says that the caller has checked the buffers against it, as
    ``SampleBuffers`` does: nothing is validated again, and ``_bias`` is the merged bias or ``None`` for none."""
    B = logits.shape[0]
    cfg, bias = config, _bias
    if cfg is None:
        cfg = SamplerConfig(temperature, top_k, top_p, eos_token_id, processors, history, keep_neutral=_force_proc)
        if cfg.history is not None:
            cfg.history.check(V)
            if out is None or out.dim() != 2 or out.shape[0] != B or out.dtype != torch.int64 \
                    or not out.is_contiguous():
                raise ValueError("sample: history constraints read the rows' histories from `out`, contiguous int64 "
                                 "[B, .]")
            if cfg.history.stop_sequences and (stop_hit is None or tuple(stop_hit.shape) != (B,)
                                               or stop_hit.dtype != torch.int32 or stop_hit.device != logits.device):
                raise ValueError("sample: stop sequences need `stop_hit`, int32 [B] on the logits' device")
            if counts is None and not cfg.processors.active:
                counts = TokenCounts(B, logits.shape[1], logits.device)    # neutral processors read nothing from it
        if cfg.processors is not None:
            if not isinstance(counts, TokenCounts) or tuple(counts.buf.shape) != tuple(logits.shape) \
                    or counts.buf.device != logits.device:
                raise ValueError("sample: processors need `counts`, a TokenCounts [B, Vp] on the logits' device")
            if bias is None:
                bias = cfg.bias(B, V, logits.shape[1], logits.device)
            if processed_out is not None and (tuple(processed_out.shape) != tuple(logits.shape)
                                              or processed_out.dtype != logits.dtype
                                              or processed_out.device != logits.device):
                raise ValueError("sample: processed_out must match the logits' shape, dtype and device")
    if isinstance(snapshot_or_state, DecodeState):
        state = snapshot_or_state
    else:
        state = DecodeState(logits.device, snapshot_or_state, rows=MAX_ROWS if logits.is_cuda else max(B, MAX_ROWS))
    if next is None:
        next = torch.zeros(B, device=logits.device, dtype=torch.int64)
    if out is None:
        out = torch.zeros(B, T0 + 1, device=logits.device, dtype=torch.int64)
    if not logits.is_cuda:
        return _sample_cpu(cfg, logits, V, state, next, out, logits_out, T0, counts, bias, processed_out, stop_hit)
    if logits.dim() != 2 or logits.dtype != _BF16 or logits.shape[1] % 8 or not logits.is_contiguous():
        raise NotImplementedError("sample: the GPU path takes contiguous bf16 logits [B, Vp] with Vp % 8 == 0")
    if B > MAX_ROWS:
        raise NotImplementedError(f"sample: at most {MAX_ROWS} rows on the GPU (got {B})")
    kw = {}
    if cfg.processors is not None:
        kw = dict(cfg._proc, counts=counts.buf, bias=bias,
                  work=torch.empty_like(logits) if processed_out is None else processed_out)
        if cfg.history is not None:
            ban, stop = cfg.history.tables(logits.device)
            kw.update(cfg._hist, ban=ban, stop=stop, stop_hit=stop_hit if stop is not None else None)
    kernels().decode_sample(logits, int(V), state.buf, next, out, logits_out, int(T0), *cfg._core, threshold_out,
                            cfg._top_p, **kw)
    return next


class SampleBuffers:
    """What a generation of ``n_new`` tokens after the prompts ``idx`` (``[B, Tin]``; ``lens``: the ``B`` prompt lengths
    of a ragged batch, or ``None``) keeps between its sampler calls, on either device: the ``DecodeState`` with the
    rows' offsets (at position ``pos``, default the longest prompt's last), ``next``, ``out`` -- ``[B, Tin + n_new]``,
    the prompts, and ``pad_token_id`` elsewhere in a ragged batch -- and ``logits_out`` (``[B, n_new, V]`` in ``dtype``
    with ``return_logits``, else ``None``).  Only when ``config`` has processors (constraints bring neutral ones):
    ``counts`` with the prompt flags set, the workspace ``work`` and the merged ``bias``; only with stop sequences:
    ``stop_hit``.  They are ``None`` otherwise.  ``Vp`` is the width of the logits that ``sample`` will be given."""

    def __init__(self, config, idx, lens, n_new, V, Vp, device, rng_state, pad_token_id=0, return_logits=False,
                 pos=None, dtype=_BF16):
        dev = torch.device(device)
        B, Tin = idx.shape
        self.config, self.V = config, int(V)
        self.T0 = T0 = Tin if lens is None else max(lens)
        self.state = DecodeState(dev, rng_state, pos=T0 - 1 if pos is None else pos, step=0,
                                 row_offsets=None if lens is None else [n - T0 for n in lens],
                                 rows=MAX_ROWS if dev.type == "cuda" else max(B, MAX_ROWS))
        self.out = _prompt_out(idx, lens, n_new, pad_token_id, dev)
        self.next = torch.zeros(B, device=dev, dtype=torch.int64)
        self.logits_out = torch.empty(B, n_new, self.V, device=dev, dtype=dtype) if return_logits else None
        self.counts = self.work = self.bias = self.stop_hit = None
        if config.processors is not None:    # allocated once; the prompt flags before the first sample
            self.counts = TokenCounts(B, Vp, dev).add_prompt(idx, self.state, T0=T0)
            self.work = torch.empty(B, Vp, device=dev, dtype=dtype)
            self.bias = config.bias(B, self.V, Vp, dev)
            if config.history is not None and config.history.stop_sequences:
                self.stop_hit = torch.full((B,), -1, device=dev, dtype=torch.int32)

    def sample(self, logits):
        """One generation step from the ``[B, Vp]`` logits of the rows' current positions; returns ``next``."""
        return sample(logits, self.V, self.state, next=self.next, out=self.out, logits_out=self.logits_out, T0=self.T0,
                      counts=self.counts, processed_out=self.work, _bias=self.bias, stop_hit=self.stop_hit,
                      config=self.config)

    def _dirty(self):
        counts = None if self.counts is None else self.counts.buf
        return [t for t in (self.state.buf, self.next, counts, self.stop_hit) if t is not None]

    def snapshot(self):
        """Copies of what a step changes besides its own output slot: state, ``next``, counts and ``stop_hit``."""
        return [t.clone() for t in self._dirty()]

    def restore(self, saved):
        for t, s in zip(self._dirty(), saved):
            t.copy_(s)


# --------------------------------------------------------------------------------------- beam search
def _prompt_out(idx, lens, n_new, pad_token_id, device):
    """The output rows of a generation before its first token: ``[B, Tin + n_new]`` int64 with the prompts in place,
    zeros after them for a batch of one length, ``pad_token_id`` everywhere else for a ragged one."""
    B, Tin = idx.shape
    if lens is None:
        out = torch.zeros(B, Tin + n_new, device=device, dtype=torch.int64)
        out[:, :Tin] = idx
        return out
    real = torch.arange(Tin, device=device)[None, :] < torch.tensor(lens, device=device)[:, None]
    out = torch.full((B, Tin + n_new), int(pad_token_id), device=device, dtype=torch.int64)
    out[:, :Tin] = torch.where(real, idx.to(device), out[:, :Tin])
    return out


def beam_step_reference(logits, V: int, num_beams: int, scores, finished, eos_token_id=None, first: bool = False,
                        return_info: bool = False):
    """One beam step (module docstring) in numpy fp64.  ``logits`` is ``[R, Vp]`` with ``R = B * num_beams`` (any
    float dtype; columns ``>= V`` never participate), ``scores`` the ``R`` cumulative log-probabilities, ``finished``
    the ``R`` flags, ``first`` says that this is step 0, where only beam 0 of every group exists.  Returns
    ``(parent, tok, score)``, each ``[B, num_beams]`` (int64, int64, fp64) in the order of the new beams.

    With ``return_info`` also a dict: ``best``, the ``num_beams + 1`` best candidate scores per group (``-inf`` where
    the group has fewer candidates), and ``gap``, per group the smallest difference between consecutive entries of
    that list -- how far the selection and its order are from changing.  Two candidates of one row with equal logits
    differ by index on either side: that pair counts as ``inf``."""
    K = int(num_beams)
    if logits.dim() != 2 or K < 1 or logits.shape[0] % K or not K <= V <= logits.shape[1]:
        raise ValueError("beam_step_reference: logits [B * num_beams, Vp] with num_beams <= V <= Vp")
    R = logits.shape[0]
    B = R // K
    eos = -1 if eos_token_id is None else int(eos_token_id)
    lg = logits.detach().float().cpu().numpy().astype(np.float64)[:, :V]
    S = np.asarray(torch.as_tensor(scores).detach().cpu().numpy(), dtype=np.float64).reshape(R)
    fin = np.asarray(torch.as_tensor(finished).detach().cpu().numpy()).astype(bool).reshape(R) & (eos >= 0)
    mx = lg.max(axis=1)
    lse = mx + np.log(np.exp(lg - mx[:, None]).sum(axis=1))
    n = min(K + 1, V)
    top = np.argsort(-lg, axis=1, kind="stable")[:, :n]          # equal logits: lowest index first
    parent, tok, score = (np.zeros((B, K), dtype=t) for t in (np.int64, np.int64, np.float64))
    best = np.full((B, K + 1), -np.inf)
    gap = np.full(B, np.inf)
    for b in range(B):
        cand = []                                                # (-score, flat index, k, v, logit or None)
        for k in range(1 if first else K):
            r = b * K + k
            if fin[r]:
                cand.append((-S[r], k * V + eos, k, eos, None))
            else:
                cand += [(-(S[r] + (lg[r, v] - lse[r])), k * V + int(v), k, int(v), lg[r, v]) for v in top[r]]
        cand.sort(key=lambda c: c[:2])
        if len(cand) < K:
            raise ValueError("beam_step_reference: fewer candidates than beams")
        for j, c in enumerate(cand[:K]):
            parent[b, j], tok[b, j], score[b, j] = c[2], c[3], -c[0]
        for j, c in enumerate(cand[:K + 1]):
            best[b, j] = -c[0]
            if j > 0:
                a = cand[j - 1]
                same = a[2] == c[2] and a[4] is not None and a[4] == c[4]
                if not same:
                    gap[b] = min(gap[b], c[0] - a[0])
    res = tuple(torch.from_numpy(x) for x in (parent, tok, score))
    return (*res, {"best": best, "gap": gap}) if return_info else res


def beam_rank_reference(scores, lengths, num_beams: int, length_penalty: float = 1.0):
    """The final ranking in numpy fp64: ``(order, ranked)``, each ``[B, num_beams]``; ``order[b, i]`` is the beam of
    rank ``i`` by ``S / len ** length_penalty`` descending, lower beam first on ties, ``ranked[b, i]`` its score."""
    K = int(num_beams)
    S = np.asarray(torch.as_tensor(scores).detach().cpu().numpy(), dtype=np.float64).reshape(-1, K)
    ln = np.asarray(torch.as_tensor(lengths).detach().cpu().numpy(), dtype=np.float64).reshape(-1, K)
    fs = S / ln ** float(length_penalty)
    order = np.argsort(-fs, axis=1, kind="stable")
    return torch.from_numpy(order), torch.from_numpy(np.take_along_axis(fs, order, axis=1))


class BeamConfig:
    """The settings of a beam search -- ``num_beams``, ``length_penalty``, ``eos_token_id`` -- validated once
    (``ValueError``).  ``active`` is False for ``num_beams == 1``: the generation then samples as without it."""

    def __init__(self, num_beams: int = 1, length_penalty: float = 1.0, eos_token_id=None, who: str = "beam search"):
        K = num_beams
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError(f"{who}: num_beams must be an integer >= 1 (got {K!r})")
        if not math.isfinite(float(length_penalty)):
            raise ValueError(f"{who}: length_penalty must be finite (got {length_penalty})")
        self.num_beams, self.length_penalty = int(K), float(length_penalty)
        self.eos_token_id = None if eos_token_id is None else _token_id(eos_token_id, f"{who}: eos_token_id")
        self._eos = -1 if self.eos_token_id is None else self.eos_token_id

    @property
    def active(self) -> bool:
        return self.num_beams > 1

    def check(self, B: int, V: int, device=None):
        """The checks that need the vocabulary: ``num_beams <= V`` (step 0 takes that many tokens of one row) and
        ``eos_token_id < V``."""
        if self.num_beams > V:
            raise ValueError(f"beam search: num_beams = {self.num_beams} exceeds the vocabulary ({V})")
        if self.eos_token_id is not None and self.eos_token_id >= V:
            raise ValueError("eos_token_id must be a token of the vocabulary")
        return self


def beam_table(B: int, num_beams: int, max_len: int, device=None):
    """The ancestor table of a beam search before its first step: uint8 ``[2, 16, stride]`` (``stride``: ``max_len``
    rounded up to a multiple of 16), entry ``[h, r, t]`` = the physical row that holds position ``t`` of the
    hypothesis living in row ``r``.  Both halves start at the group's first row ``(r // K) * K``, where the prefill
    stores the prompt's K and V once.  Layout and update rule: ``PdeBeamTable`` in ``pde_decode.h``."""
    K, R = int(num_beams), int(B) * int(num_beams)
    if R > MAX_ROWS:
        raise NotImplementedError(f"beam search: B * num_beams <= {MAX_ROWS} rows (got {R})")
    first = (torch.arange(MAX_ROWS) // K * K).clamp(max=max(R - 1, 0)).to(torch.uint8)
    stride = -(-int(max_len) // 16) * 16
    return first[None, :, None].repeat(2, 1, stride).contiguous().to(torch.device("cpu" if device is None else device))


class BeamBuffers:
    """What a GPU beam search of ``n_new`` tokens after the prompts ``idx`` (``[B, Tin]``; ``lens`` as for
    ``SampleBuffers``) keeps between its steps, all on the device, for the ``R = B * num_beams`` physical rows
    ``r = b * K + k``: the ``DecodeState`` (every row of a group carries the group's offset; the finished flags are the
    rows'), ``next`` (``[R]``), ``score`` (``S``, fp32 ``[R]``), ``len`` (int32 ``[R]``), the ancestor ``table`` for a
    cache of ``max_len`` positions, the traces ``tok`` / ``parent`` / ``score_trace`` (``[n_new, R]``: what every step
    chose), the selection's workspaces and ``logits_out`` (``[R, n_new, V]`` with ``return_logits``).  ``sample(logits)``
    is one beam step; ``finalize()`` ranks the rows and returns ``(out [B, K, Tin + n_new], scores [B, K])``."""

    def __init__(self, config: BeamConfig, idx, lens, n_new, V, Vp, device, max_len, pad_token_id=0,
                 return_logits=False, pos=None):
        dev = torch.device(device)
        B, Tin = idx.shape
        K = config.num_beams
        R = B * K
        if R > MAX_ROWS:
            raise NotImplementedError(f"beam search: B * num_beams <= {MAX_ROWS} rows on the GPU (got {B} * {K})")
        config.check(B, V)
        self.config, self.V, self.B, self.K, self.n_new, self.max_len = config, int(V), B, K, int(n_new), int(max_len)
        self.T0 = T0 = Tin if lens is None else max(lens)
        offs = None if lens is None else [n - T0 for n in lens for _ in range(K)]
        self.state = DecodeState(dev, None, pos=T0 - 1 if pos is None else pos, step=0, row_offsets=offs)
        self.next = torch.zeros(R, device=dev, dtype=torch.int64)
        self.score = torch.zeros(R, device=dev, dtype=torch.float32)
        self.len = torch.zeros(R, device=dev, dtype=torch.int32)
        self.table = beam_table(B, K, max_len, dev)
        self.tok = torch.zeros(n_new, R, device=dev, dtype=torch.int32)
        self.parent = torch.zeros(n_new, R, device=dev, dtype=torch.int32)
        self.score_trace = torch.zeros(n_new, R, device=dev, dtype=torch.float32)
        self._cand = (torch.zeros(R, K, device=dev, dtype=torch.float32), torch.zeros(R, K, device=dev, dtype=torch.int32))
        self.logits_out = torch.zeros(R, n_new, self.V, device=dev, dtype=_BF16) if return_logits else None
        self.out = _prompt_out(idx, lens, n_new, pad_token_id, dev)[:, None, :].repeat(1, K, 1).contiguous()
        self.scores = torch.zeros(B, K, device=dev, dtype=torch.float32)

    def sample(self, logits):
        """One beam step from the ``[R, Vp]`` logits of the rows' current positions; returns ``next``."""
        return beam_step(logits, self)

    def finalize(self, n_steps=None):
        """To be called after the last step (``n_steps`` of them, default ``n_new``; nothing is read on the host)."""
        n = self.n_new if n_steps is None else int(n_steps)
        kernels().beam_finalize(self.state.buf, self.score, self.len, self.tok, self.parent, self.out, self.scores,
                                self.T0, n, self.config.length_penalty)
        return self.out, self.scores

    def _dirty(self):
        return [self.state.buf, self.next, self.score, self.len]

    def snapshot(self):
        """Copies of what a step changes besides the trace slots and the table half it writes: state (position, step,
        finished flags), ``next``, ``S`` and ``len``."""
        return [t.clone() for t in self._dirty()]

    def restore(self, saved):
        for t, s in zip(self._dirty(), saved):
            t.copy_(s)


def beam_step(logits, buffers: BeamBuffers):
    """One beam step on the device (definition in the module docstring; ``beam_step_reference`` is its fp64 twin):
    a block per row finds ``lse`` and the row's ``K`` best logits, a block per prompt merges the group's candidates
    and writes ``next``, ``S``, ``len``, the finished flags, the trace slots of the state's step and the other half
    of the ancestor table, and a one-thread tail advances position and step.  Returns ``next``."""
    b = buffers
    if not logits.is_cuda:
        raise NotImplementedError("beam_step: the device step runs on the GPU; the CPU definition is "
                                  "beam_step_reference")
    if logits.dim() != 2 or logits.dtype != _BF16 or logits.shape[1] % 8 or not logits.is_contiguous() \
            or logits.shape[0] != b.B * b.K:
        raise NotImplementedError("beam_step: contiguous bf16 logits [B * num_beams, Vp] with Vp % 8 == 0")
    kernels().beam_step(logits, b.V, b.K, b.state.buf, b.next, b.score, b.len, b._cand[0], b._cand[1], b.table,
                        b.max_len, b.tok, b.parent, b.score_trace, b.logits_out, b.config._eos)
    return b.next
