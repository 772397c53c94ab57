"""GPT-2 (124M, "small") in bf16 over the framework's transformer ops.

Driver-added config of BASELINE.json ("GPT-2-small transformer DDP 8xMI355X: large grad buckets,
MFMA GEMM + fused Adam"); the reference itself has no transformer (survey §2.5).  Architecture =
GPT-2 small: 12 layers, 12 heads x 64, d_model 768, context 1024, vocab 50257 padded to 50304 (a
multiple of 128, for GEMM tiling), pre-LayerNorm blocks, tanh-GELU MLP (4x), tied token embedding /
LM head, learned positions.  Parameter names follow the common GPT-2 checkpoint layout
(``transformer.wte.weight``, ``transformer.h.{i}.attn.c_attn.weight`` [3C, C], ...); weights are
stored bf16 (the fused AdamW keeps the fp32 master copy).

Dropout (``embd_pdrop`` / ``attn_pdrop`` / ``resid_pdrop``, all 0.0 by default) runs inside the
kernels from a counter-based device RNG (``ops/rng.py``): ``GPT.rng`` draws one snapshot per training
forward, and every site of that forward and its backward regenerates its mask from it.  Sites are
numbered: embedding 0; layer ``l`` attention probabilities ``1 + 3l``, attention-projection output
``2 + 3l``, MLP output ``3 + 3l``.

Packed sequences (``GPT.forward(idx, targets, doc_ids=)``): rows that hold several concatenated documents.
``ops.doc_bounds`` turns the ids into per-position document bounds once per forward, on the device; the
attention of every block masks keys outside the query's document (and skips key tiles no query of a block
can see) and the embedding takes the position inside the document.  Generation never uses it.

Generation (``GPT.generate``): the prompt goes once through the training kernels and fills a KV cache;
every further token is one decode step over ``ops/decode.py`` (``DecodeSession``) whose per-token state
lives on the device, so the step is captured once and replayed.  It uses a ``DeviceRNG`` of its own, never
``GPT.rng``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as tnn

from ..ops import decode as D
from ..ops import transformer as T
from ..ops.rng import DeviceRNG


@dataclass
class GPTConfig:
    block_size: int = 1024
    vocab_size: int = 50257
    padded_vocab: int = 50304
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    ln_eps: float = 1e-5
    embd_pdrop: float = 0.0
    attn_pdrop: float = 0.0
    resid_pdrop: float = 0.0


class _LN(tnn.Module):
    def __init__(self, C, eps):
        super().__init__()
        self.weight = tnn.Parameter(torch.ones(C))
        self.bias = tnn.Parameter(torch.zeros(C))
        self.eps = eps

    def forward(self, x):
        return T.layer_norm(x, self.weight, self.bias, self.eps)


class _Linear(tnn.Module):
    def __init__(self, fin, fout, std):
        super().__init__()
        self.weight = tnn.Parameter(torch.empty(fout, fin).normal_(0.0, std))
        self.bias = tnn.Parameter(torch.zeros(fout))

    def forward(self, x):
        return T.linear(x, self.weight, self.bias)


class _Attn(tnn.Module):
    def __init__(self, cfg: GPTConfig):
        super().__init__()
        C = cfg.n_embd
        self.n_head = cfg.n_head
        self.attn_pdrop = cfg.attn_pdrop
        self.c_attn = _Linear(C, 3 * C, 0.02)
        self.c_proj = _Linear(C, C, 0.02 / math.sqrt(2 * cfg.n_layer))

    def forward(self, x, snap=None, site=0, doc_bounds=None):
        if doc_bounds is not None:      # packed sequences (ops.doc_bounds), with or without dropout
            p = 0.0 if snap is None else self.attn_pdrop
            return self.c_proj(T.causal_attention(self.c_attn(x), self.n_head, p, snap, site, doc_bounds=doc_bounds))
        if snap is None or self.attn_pdrop == 0.0:
            return self.c_proj(T.causal_attention(self.c_attn(x), self.n_head))
        return self.c_proj(T.causal_attention(self.c_attn(x), self.n_head, self.attn_pdrop, snap, site))


class _MLP(tnn.Module):
    def __init__(self, cfg: GPTConfig):
        super().__init__()
        C = cfg.n_embd
        self.c_fc = _Linear(C, 4 * C, 0.02)
        self.c_proj = _Linear(4 * C, C, 0.02 / math.sqrt(2 * cfg.n_layer))

    def forward(self, x):
        return T.mlp(x, self.c_fc.weight, self.c_fc.bias, self.c_proj.weight, self.c_proj.bias)


class Block(tnn.Module):
    def __init__(self, cfg: GPTConfig, layer_idx: int = 0):
        super().__init__()
        self.layer_idx = layer_idx
        self.resid_pdrop = cfg.resid_pdrop
        self.ln_1 = _LN(cfg.n_embd, cfg.ln_eps)
        self.attn = _Attn(cfg)
        self.ln_2 = _LN(cfg.n_embd, cfg.ln_eps)
        self.mlp = _MLP(cfg)

    def forward(self, x, delta=None):
        return sum(self.forward_deferred(x, delta))

    def forward_deferred(self, x, delta=None, snap=None, doc_bounds=None):
        """(residual, mlp_out) with the block output = residual + mlp_out left unsummed, so the next
        LayerNorm adds it inside its kernel.  ``delta`` is the previous block's deferred mlp_out.
        (residual, LN(x)) come from one op: the residual-gradient add is fused into the LN backward.
        ``snap`` (an RNG snapshot of this forward) turns dropout on: the returned mlp_out is still
        undropped -- whoever adds it drops it under this layer's site ``3 + 3l``, as this block does
        with the ``delta`` it is handed.  ``doc_bounds`` (``ops.doc_bounds``) masks attention per document."""
        if snap is not None:
            return self._forward_deferred_drop(x, delta, snap, doc_bounds)
        if delta is None:
            x, h = T.layer_norm_residual(x, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        else:
            x, h = T.add_layer_norm_residual(x, delta, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        x, h = T.add_layer_norm_residual(x, self.attn(h, doc_bounds=doc_bounds), self.ln_2.weight, self.ln_2.bias,
                                         self.ln_2.eps)
        return x, self.mlp(h)

    def forward_deferred_qkv(self, x, delta=None):
        """``forward_deferred`` without dropout that also returns this layer's c_attn output
        ``[B, T, 3C]``: the prefill of ``GPT.generate`` fills the KV cache from it."""
        if delta is None:
            x, h = T.layer_norm_residual(x, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        else:
            x, h = T.add_layer_norm_residual(x, delta, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        qkv = self.attn.c_attn(h)
        a = self.attn.c_proj(T.causal_attention(qkv, self.attn.n_head))
        x, h = T.add_layer_norm_residual(x, a, self.ln_2.weight, self.ln_2.bias, self.ln_2.eps)
        return x, self.mlp(h), qkv

    def decode_deferred(self, x, delta, cache, state):
        """One-token ``forward_deferred`` over the decode kernels: ``x`` / ``delta`` are ``[B, C]``, the
        new K and V are appended to ``cache`` at the position held by ``state``."""
        if delta is None:
            x, h = T.layer_norm_residual(x, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        else:
            x, h = T.add_layer_norm_residual(x, delta, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        qkv = D.skinny_linear(h, self.attn.c_attn.weight, self.attn.c_attn.bias)
        a = D.decode_attention(qkv, cache, self.layer_idx, state)
        a = D.skinny_linear(a, self.attn.c_proj.weight, self.attn.c_proj.bias)
        x, h = T.add_layer_norm_residual(x, a, self.ln_2.weight, self.ln_2.bias, self.ln_2.eps)
        f = D.skinny_linear(h, self.mlp.c_fc.weight, self.mlp.c_fc.bias, gelu=True)
        return x, D.skinny_linear(f, self.mlp.c_proj.weight, self.mlp.c_proj.bias)

    def _forward_deferred_drop(self, x, delta, snap, doc_bounds=None):
        l, p = self.layer_idx, self.resid_pdrop
        if delta is None:
            x, h = T.layer_norm_residual(x, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        else:
            x, h = T.add_dropout_layer_norm_residual(x, delta, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps,
                                                     p, snap, 3 * l)          # = 3 + 3(l - 1)
        x, h = T.add_dropout_layer_norm_residual(x, self.attn(h, snap, 1 + 3 * l, doc_bounds), self.ln_2.weight,
                                                 self.ln_2.bias, self.ln_2.eps, p, snap, 2 + 3 * l)
        return x, self.mlp(h)


class _Transformer(tnn.Module):
    def __init__(self, cfg: GPTConfig):
        super().__init__()
        self.wte = tnn.Embedding(cfg.padded_vocab, cfg.n_embd)
        self.wpe = tnn.Embedding(cfg.block_size, cfg.n_embd)
        tnn.init.normal_(self.wte.weight, 0.0, 0.02)
        tnn.init.normal_(self.wpe.weight, 0.0, 0.01)
        self.h = tnn.ModuleList([Block(cfg, l) for l in range(cfg.n_layer)])
        self.ln_f = _LN(cfg.n_embd, cfg.ln_eps)


class GPT(tnn.Module):
    def __init__(self, cfg: GPTConfig = GPTConfig()):
        super().__init__()
        self.config = cfg
        self.transformer = _Transformer(cfg)
        self._rng = None          # DeviceRNG, created on first use (plain attribute: not a buffer)
        self._rng_init = (0, 0)

    @property
    def rng(self) -> DeviceRNG:
        """The model's dropout RNG, on the parameters' device.  Checkpoint it with
        ``model.rng.state_dict()`` / ``load_state_dict()``; it is not part of ``model.state_dict()``."""
        dev = self.transformer.wte.weight.device
        if self._rng is None:
            self._rng = DeviceRNG(self._rng_init[0], self._rng_init[1], device=dev)
        elif self._rng.device != dev:
            self._rng.to(dev)
        return self._rng

    def seed_dropout(self, seed: int, stream: int = 0):
        """Seed the dropout RNG (draw number back to 0).  ``stream`` is the data-parallel rank: one
        seed, different masks per replica."""
        self._rng_init = (int(seed), int(stream))
        if self._rng is not None:
            self._rng.manual_seed(seed, stream)
        return self

    def dropout_active(self) -> bool:
        c = self.config
        return self.training and (c.embd_pdrop > 0.0 or c.attn_pdrop > 0.0 or c.resid_pdrop > 0.0)

    def forward(self, idx, targets=None, doc_ids=None, *, ignore_index=None, loss_mask=None, mask_doc_ends=False,
                reduction="mean", denom=None, label_smoothing=0.0, z_loss=0.0, loss_weights=None):
        """Logits ``[B, T, V]``, or the mean cross-entropy against ``targets``.

        ``doc_ids`` (an integer ``[B, T]`` tensor on the model's device) marks packed rows: a document
        begins at ``t = 0`` and wherever ``doc_ids[b, t] != doc_ids[b, t - 1]``.  Every token then attends
        to its own document only and takes the learned position of its offset inside that document, so
        each document is computed as if it stood alone at the start of a row.  ``None`` is the call as it
        was.

        By default the loss is the mean over all ``B * T`` targets, the one after each document's last token
        included.  The keywords select the masked loss (``ops.loss_targets``, ``ops.transformer.lm_head_loss``):
        targets equal to ``ignore_index``, positions where ``loss_mask`` (bool / uint8 ``[B, T]``) is 0 and,
        with ``mask_doc_ends=True`` (needs ``doc_ids``), the target after each document's last token do not
        count, and the mean divides by the number of targets that do.  The target of the row's last position
        ``t = T - 1`` is kept under ``mask_doc_ends``: whether its document goes on past the row cannot be
        known from ``doc_ids``.  A batch without one valid target gives loss 0 and zero gradients, not NaN.
        ``denom`` (an fp32 device scalar) replaces the count as the denominator, for a global mean over
        data-parallel ranks or accumulated micro-batches; ``reduction`` is ``"mean"``, ``"sum"`` or
        ``"none"`` (per-position losses, no gradient).  The valid count stays on the device, so a captured
        step follows every batch.

        ``label_smoothing`` (in ``[0, 1)``), ``z_loss`` (``>= 0``, the coefficient of ``lse^2``) and
        ``loss_weights`` (a floating ``[B, T]`` tensor, one weight per target) select the smoothed and weighted
        loss defined in ``ops.transformer.lm_head_loss``.  The mean still divides by the number of valid
        targets, whatever their weights (pass the weights' sum as ``denom`` for a weighted mean).  The two
        numbers are frozen into a captured step; the weights are device data and follow every replay."""
        if mask_doc_ends and doc_ids is None:
            raise ValueError("GPT.forward: mask_doc_ends=True needs doc_ids")
        t = self.transformer
        # computed once, on the device, and handed to the embedding and to every block
        bounds = None if doc_ids is None else T.doc_bounds(doc_ids)
        # one draw per training forward, before its first site; none at all when dropout is off
        snap = self.rng.next() if self.dropout_active() else None
        if bounds is not None:
            x = T.embedding(idx, t.wte.weight, t.wpe.weight, 0.0 if snap is None else self.config.embd_pdrop, snap, 0,
                            doc_bounds=bounds)
        elif snap is None:
            x = T.embedding(idx, t.wte.weight, t.wpe.weight)
        else:
            x = T.embedding(idx, t.wte.weight, t.wpe.weight, self.config.embd_pdrop, snap, 0)
        delta = None
        for blk in t.h:
            x, delta = blk.forward_deferred(x, delta, snap, bounds)
        if delta is None:
            x = t.ln_f(x)
        elif snap is None:   # last block's residual add fused into ln_f (the summed stream itself is not needed)
            x = T.add_layer_norm_residual(x, delta, t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
        else:   # no site of its own: the last block's MLP output, dropped under that layer's site
            x = T.add_dropout_layer_norm_residual(x, delta, t.ln_f.weight, t.ln_f.bias, t.ln_f.eps,
                                                  self.config.resid_pdrop, snap, 3 * len(t.h))[1]
        if targets is None:
            return T.lm_logits(x, t.wte.weight, self.config.vocab_size)
        return T.lm_head_loss(x, t.wte.weight, targets, self.config.vocab_size, ignore_index=ignore_index,
                              loss_mask=loss_mask, doc_bounds=bounds if mask_doc_ends else None,
                              mask_doc_ends=mask_doc_ends, reduction=reduction, denom=denom,
                              label_smoothing=label_smoothing, z_loss=z_loss, loss_weights=loss_weights)

    # ------------------------------------------------------------------------------- generation
    def generate(self, idx, max_new_tokens, temperature=1.0, top_k=None, seed=None, generator=None,
                 eos_token_id=None, use_graph=True, return_logits=False, top_p=None, prompt_lens=None,
                 pad_token_id=0, _after_prefill=None, repetition_penalty=1.0, frequency_penalty=0.0,
                 presence_penalty=0.0, logit_bias=None, suppress_tokens=None, min_new_tokens=0,
                 no_repeat_ngram_size=0, bad_words_ids=None, stop_sequences=None):
        """Sample ``max_new_tokens`` tokens after the prompts ``idx`` ``[B, T0]`` (``T0 >= 1``).

        Returns ``[B, T0 + max_new_tokens]`` int64, and with ``return_logits`` also the logits every token
        was sampled from, ``[B, max_new_tokens, V]`` indexed by step (bf16 on the GPU, the model's dtype on
        the CPU).  Sampling is defined in ``ops/decode.py``: ``temperature == 0`` is greedy (lowest index
        among equal maxima), ``top_k`` keeps ties at its threshold, and ``top_p`` in ``(0, 1]`` (``None`` and
        1.0: off; ignored when greedy) then keeps the smallest set of largest logit values, ties kept, whose
        mass inside the top-k set reaches ``top_p``.

        ``prompt_lens`` (a list or int tensor of ``B`` lengths, read once on the host) makes the batch
        ragged: ``idx`` is right-padded, row ``b``'s prompt is ``idx[b, :len_b]`` with
        ``1 <= len_b <= T0`` and whatever lies beyond is ignored.  Every row starts at position 0 and
        generates exactly ``max_new_tokens`` tokens at positions ``len_b .. len_b + max_new_tokens - 1``; in
        the output they follow the prompt directly, and the rest of the row is ``pad_token_id``.  No
        attention mask is involved: attention is causal, so a pad column never reaches a real position.
        One RNG draw number per generated token, whatever the lengths.  The random numbers come from ``generator`` (a
        ``DeviceRNG`` whose draw number advances by ``max_new_tokens``; checkpoint it with
        ``state_dict()``) or a fresh one from ``seed``; ``model.rng``, the dropout generator, is never
        touched.  A row that emits ``eos_token_id`` keeps emitting it.  Runs without gradients and with
        dropout off, and restores the module's training flag.

        ``repetition_penalty`` (``> 0``, HF / vLLM: logits of tokens seen in the prompt or the output are
        divided by it when positive, multiplied when not), ``frequency_penalty`` and ``presence_penalty``
        (OpenAI / vLLM: ``f * count + p * [count > 0]`` is subtracted, counting generated tokens only),
        ``logit_bias`` (fp32 ``[V]`` or ``[B, V]`` on the model's device, added; ``-inf`` bans a token),
        ``suppress_tokens`` (token ids that never appear) and ``min_new_tokens`` (no ``eos_token_id`` before
        that step) are the logit processors defined in ``ops/decode.py``, applied in that order before the
        sampling above, one value for the whole batch.  On the GPU they run inside the sampler kernel on a
        per-row history of token counts that lives on the device, so they work under graph replay.  With all
        of them at their defaults nothing is allocated and the sampler runs as before.  ``return_logits``
        keeps returning the raw model logits, not the processed ones.

        ``no_repeat_ngram_size`` (``n`` in 1 .. 8: no n-gram occurs twice in a row's prompt plus output, as Hugging
        Face's processor), ``bad_words_ids`` (token lists that never appear as a sequence; a single token is never
        emitted) and ``stop_sequences`` (token lists; a row whose generated tokens end in one becomes finished and
        emits ``eos_token_id``, which they need, from the next step on; the sequence stays in the output) are the
        history constraints defined in ``ops/decode.py``.  They match each row's history -- its columns of the
        output buffer -- inside the sampler kernel, so they too work under graph replay, and with all three at
        their defaults nothing changes.  Bans apply after the bias and before ``min_new_tokens``.

        GPU (bf16, ``B <= 16``): the prompt, padded to a multiple of 128, goes through the training
        kernels once and fills the KV cache; every further token is one decode step -- about a hundred
        small launches that read position, output slot, RNG draw and finished flags from a device state
        buffer.  With ``use_graph`` that step is captured once and replayed per token: no host work and no
        host read until the result.  CPU: the plain definition, a full forward per token.

        ``T0 + max_new_tokens`` (``max(prompt_lens) + max_new_tokens`` for a ragged batch) must not exceed
        ``block_size`` (learned absolute positions: no sliding window)."""
        cfg = self.config
        if idx.dim() != 2 or idx.shape[1] < 1:
            raise ValueError("generate: idx must be [B, T0] with T0 >= 1")
        B, T0 = idx.shape
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be >= 1")
        lens = None
        if prompt_lens is not None:
            lens = [int(n) for n in (prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
            if len(lens) != B:
                raise ValueError(f"generate: prompt_lens holds {len(lens)} lengths for {B} rows")
            if min(lens) < 1 or max(lens) > T0:
                raise ValueError(f"generate: every prompt length must be in 1 .. {T0} (got {lens})")
        Tlong = T0 if lens is None else max(lens)
        if Tlong + max_new_tokens > cfg.block_size:
            raise ValueError(f"generate: T0 + max_new_tokens = {Tlong + max_new_tokens} exceeds block_size "
                             f"{cfg.block_size} (positions are learned and absolute: no sliding window)")
        if not 0 <= int(pad_token_id) < cfg.vocab_size:
            raise ValueError("generate: pad_token_id must be a token of the vocabulary")
        if temperature < 0:
            raise ValueError("generate: temperature must be >= 0")
        if top_k is not None and top_k < 1:
            raise ValueError("generate: top_k must be >= 1")
        D.check_top_p(top_p, "generate")
        if eos_token_id is not None and not 0 <= eos_token_id < cfg.vocab_size:
            raise ValueError("generate: eos_token_id must be a token of the vocabulary")
        dev = self.transformer.wte.weight.device
        procs = D.LogitProcessors(repetition_penalty, frequency_penalty, presence_penalty, logit_bias, suppress_tokens,
                                  min_new_tokens, eos_token_id).check(B, cfg.vocab_size, dev)
        procs = procs if procs.active else None          # neutral settings: the calls below are what they were
        hist = D.HistoryConstraints(no_repeat_ngram_size, bad_words_ids, stop_sequences,
                                    eos_token_id).check(cfg.vocab_size)
        hist = hist if hist.active else None
        if generator is None:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            generator = DeviceRNG(seed, device=dev)
        else:
            generator.to(dev)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                run = self._generate_gpu if dev.type == "cuda" else self._generate_cpu
                return run(idx.to(dev).long(), max_new_tokens, float(temperature), top_k, generator, eos_token_id,
                           use_graph, return_logits, _after_prefill, top_p, lens, int(pad_token_id), procs, hist)
        finally:
            self.train(was_training)

    def _generate_cpu(self, idx, n_new, temperature, top_k, generator, eos, use_graph, return_logits, _after_prefill,
                      top_p=None, lens=None, pad=0, procs=None, hist=None):
        V = self.config.vocab_size
        if lens is not None:
            return self._generate_cpu_ragged(idx, n_new, temperature, top_k, generator, eos, return_logits, top_p,
                                             lens, pad, procs, hist)
        seq = idx
        fin = torch.zeros(idx.shape[0], dtype=torch.bool)
        kept = []
        sample = None
        if procs is not None or hist is not None:
            sample = _CpuProcSampler(procs, idx, None, V, generator, temperature, top_k, eos, top_p, hist, n_new)
        for _ in range(n_new):
            logits = self(seq)[:, -1]
            if sample is not None:
                tok = sample(logits)
            else:
                tok = D.sample_reference(logits, V, generator.next(), temperature, top_k, top_p=top_p)
                if eos is not None:
                    tok = torch.where(fin, torch.full_like(tok, eos), tok)
                    fin = fin | (tok == eos)
            seq = torch.cat([seq, tok[:, None]], dim=1)
            if return_logits:
                kept.append(logits)
        return (seq, torch.stack(kept, dim=1)) if return_logits else seq

    def _generate_cpu_ragged(self, idx, n_new, temperature, top_k, generator, eos, return_logits, top_p, lens, pad,
                             procs=None, hist=None):
        """One right-padded forward per token; row ``b``'s logits are row ``len_b + s - 1`` of it (causal:
        independent of what follows), gathered into ``[B, V]`` for one sampler call per step, so the
        Philox row index is ``b`` as on the GPU."""
        V = self.config.vocab_size
        B, T0 = idx.shape
        Tl = max(lens)
        ln = torch.tensor(lens, dtype=torch.int64)
        rows = torch.arange(B)
        real = torch.arange(T0)[None, :] < ln[:, None]
        out = torch.full((B, T0 + n_new), pad, dtype=torch.int64)
        out[:, :T0] = torch.where(real, idx, out[:, :T0])
        seq = torch.zeros(B, Tl + n_new, dtype=torch.int64)        # what the model sees: pad columns hold token 0
        seq[:, :Tl] = torch.where(real[:, :Tl], idx[:, :Tl], seq[:, :Tl])
        fin = torch.zeros(B, dtype=torch.bool)
        kept = []
        sample = None
        if procs is not None or hist is not None:
            sample = _CpuProcSampler(procs, idx, lens, V, generator, temperature, top_k, eos, top_p, hist, n_new)
        for s in range(n_new):
            logits = self(seq[:, :Tl + s])[rows, ln + s - 1]
            if sample is not None:
                tok = sample(logits)
            else:
                tok = D.sample_reference(logits, V, generator.next(), temperature, top_k, top_p=top_p)
                if eos is not None:
                    tok = torch.where(fin, torch.full_like(tok, eos), tok)
                    fin = fin | (tok == eos)
            seq[rows, ln + s] = tok
            out[rows, ln + s] = tok
            if return_logits:
                kept.append(logits)
        return (out, torch.stack(kept, dim=1)) if return_logits else out

    def _generate_gpu(self, idx, n_new, temperature, top_k, generator, eos, use_graph, return_logits, _after_prefill,
                      top_p=None, lens=None, pad=0, procs=None, hist=None):
        ses = DecodeSession(self, idx, n_new, temperature, top_k, generator.state, eos, return_logits, top_p=top_p,
                            prompt_lens=lens, pad_token_id=pad, processors=procs, history=hist)
        if _after_prefill is not None:
            _after_prefill(ses.cache)
        if n_new > 1 and use_graph:
            graph = ses.capture()
            for _ in range(n_new - 1):
                graph.replay()
        else:
            for _ in range(n_new - 1):
                ses.step()
        generator.state.copy_(ses.state.rng)      # the draw number advanced by n_new, on the device
        return (ses.out, ses.logits_out) if return_logits else ses.out

    def num_params(self, non_embedding: bool = False):
        n = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n -= self.transformer.wpe.weight.numel()
        return n

    def decay_groups(self, weight_decay: float):
        """AdamW groups: matrices/embeddings decay, biases and LayerNorm parameters do not."""
        decay = [p for n, p in self.named_parameters() if p.dim() >= 2]
        nodecay = [p for n, p in self.named_parameters() if p.dim() < 2]
        return [{"params": decay, "weight_decay": weight_decay}, {"params": nodecay, "weight_decay": 0.0}]

    def flops_per_token(self) -> float:
        """Training FLOPs per token (6N for the matmul weights + causal attention, PaLM appendix B)."""
        c = self.config
        N = self.num_params() - self.transformer.wpe.weight.numel()
        return 6 * N + 6 * c.n_layer * c.n_embd * c.block_size  # causal: half of 12*L*C*T


class _CpuProcSampler:
    """The sampling step of the CPU generations when logit processors are on: ``ops.sample`` on a CPU
    ``DecodeState`` and ``TokenCounts``, the path the GPU takes, so that eos, the step that ``min_new_tokens``
    compares with and the counts are kept in one place.  Advances ``generator`` by one draw per call.

    With history constraints (``hist``) it also keeps what they read: an output buffer that holds the prompts and
    receives the tokens, the rows' offsets in the state, and ``stop_hit``."""

    def __init__(self, procs, idx, lens, V, generator, temperature, top_k, eos, top_p, hist=None, n_new=0):
        self.B, self.V, self.generator = idx.shape[0], V, generator
        self.procs = D.LogitProcessors(eos_token_id=eos) if procs is None else procs
        self.args = (temperature, top_k, eos)
        self.top_p = top_p
        self.state = D.DecodeState("cpu", generator.state)
        self.counts = None
        self.prompt = (idx, lens)
        self.hist, self.kw, self.stop_hit = hist, {}, None
        if hist is not None:
            T0 = idx.shape[1] if lens is None else max(lens)
            self.state.reset(generator.state, row_offsets=None if lens is None else [n - T0 for n in lens])
            out = torch.zeros(self.B, T0 + n_new, dtype=torch.int64)
            out[:, :T0] = idx[:, :T0]                 # columns >= len_b are overwritten before they are history
            if hist.stop_sequences:
                self.stop_hit = torch.full((self.B,), -1, dtype=torch.int32)
            self.kw = dict(history=hist, out=out, T0=T0, stop_hit=self.stop_hit)

    def __call__(self, logits):
        if self.counts is None:          # the logits' width is the counts' width
            self.counts = D.TokenCounts(self.B, logits.shape[1]).add_prompt(*self.prompt)
            self.bias = self.procs.bias(self.B, self.V, logits.shape[1])
            if self.hist is not None:
                self.bias = self.hist.merge_bias(self.bias, self.V, logits.shape[1])
        tok = D.sample(logits, self.V, self.state, *self.args, top_p=self.top_p, processors=self.procs,
                       counts=self.counts, _bias=self.bias, **self.kw).clone()
        self.generator.state.copy_(self.state.rng)
        return tok


class DecodeSession:
    """One GPU generation of ``GPT.generate``: the KV cache, the device state and the static buffers.

    The constructor runs the prefill -- the prompt, padded to a multiple of 128, through the training
    kernels, filling the cache -- and samples the first token.  With ``prompt_lens`` the window is that of
    the longest prompt, and the device state carries every row's offset from it.  ``step()`` then generates
    one token per call and touches nothing on the host that changes between tokens, so ``capture()`` can
    record it once and every ``replay()`` of the returned graph yields the next token.  Call under
    ``torch.no_grad()`` with the model in eval mode (``GPT.generate`` does).

    The logit processors (``processors``, an ``ops.LogitProcessors``, or the six keywords of ``GPT.generate``):
    when any of them is on, the session allocates the token counts, the sampler's workspace and the padded
    bias once, sets the prompt flags before the prefill's sample, and every sample passes them; the counts
    live on the device and the sampler advances them, so a replayed step sees the history.  When none is on,
    ``counts``, ``work`` and ``bias`` stay ``None`` and the sampler is called exactly as without them.

    The history constraints (``history``, an ``ops.HistoryConstraints``, or the three keywords of ``GPT.generate``)
    read the rows' histories from ``out``.  When any is on, the session allocates what the processors need (they
    share the kernel's prologue), with stop sequences also ``stop_hit`` (int32 ``[B]`` on the device: ``-1``, or
    the index of the stop sequence that finished the row), and passes ``history`` on every sample, the prefill's
    included.  When none is on, ``history`` and ``stop_hit`` stay ``None``."""

    def __init__(self, model, idx, n_new, temperature=1.0, top_k=None, rng_state=None, eos=None,
                 return_logits=False, top_p=None, prompt_lens=None, pad_token_id=0, processors=None,
                 repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None,
                 suppress_tokens=None, min_new_tokens=0, history=None, no_repeat_ngram_size=0, bad_words_ids=None,
                 stop_sequences=None):
        cfg, t = model.config, model.transformer
        dev = idx.device
        B, Tin = idx.shape
        D.check_top_p(top_p, "generate")
        if processors is None:
            processors = D.LogitProcessors(repetition_penalty, frequency_penalty, presence_penalty, logit_bias,
                                           suppress_tokens, min_new_tokens, eos)
        processors.check(B, cfg.vocab_size, dev)
        # inactive processors: no counts, no workspace, and _sample calls exactly what it called without them
        if history is None:
            history = D.HistoryConstraints(no_repeat_ngram_size, bad_words_ids, stop_sequences, eos)
        history.check(cfg.vocab_size)
        if history.stop_sequences and history.eos_token_id != eos:
            raise ValueError("generate: the stop sequences' eos_token_id differs from eos")
        self.history = history if history.active else None
        self.processors = processors if processors.active or self.history is not None else None
        self.counts = self.work = self.bias = self.stop_hit = None
        if prompt_lens is None:
            lens = None
            T0 = Tin
        else:
            lens = [int(n) for n in (prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
            if len(lens) != B or min(lens) < 1 or max(lens) > Tin:
                raise ValueError(f"generate: prompt_lens must hold {B} lengths in 1 .. {Tin} (got {lens})")
            T0 = max(lens)                       # the longest prompt: window, cache length and base position
        if T0 + n_new > cfg.block_size:
            raise ValueError(f"generate: T0 + max_new_tokens = {T0 + n_new} exceeds block_size {cfg.block_size}")
        wte, wpe = t.wte.weight, t.wpe.weight
        if B > D.MAX_ROWS:
            raise NotImplementedError(f"generate: at most {D.MAX_ROWS} sequences on the GPU (got {B})")
        if wte.dtype != torch.bfloat16:
            raise NotImplementedError("generate: the GPU path is bf16")
        Tpad = min(-(-T0 // 128) * 128, cfg.block_size)
        if Tpad % 128:
            raise NotImplementedError("generate: the prefill needs a window that is a multiple of 128 "
                                      f"(block_size {cfg.block_size} caps it at {Tpad})")
        self.model, self.T0, self.V = model, T0, cfg.vocab_size
        self.sampling = (float(temperature), top_k, eos, top_p)
        # prefill: the training kernels over the padded prompt (causal: the pad never reaches positions < T0)
        self.cache = D.KVCache(cfg, B, T0 + n_new, dev)
        idx_pad = torch.zeros(B, Tpad, device=dev, dtype=torch.int64)
        if lens is None:
            idx_pad[:, :T0] = idx
        else:                                    # columns >= len_b hold token 0, whatever idx holds there
            ln = torch.tensor(lens, device=dev, dtype=torch.int64)
            real = torch.arange(Tin, device=dev)[None, :] < ln[:, None]
            idx_pad[:, :T0] = torch.where(real[:, :T0], idx[:, :T0], idx_pad[:, :T0])
        x, delta = T.embedding(idx_pad, wte, wpe), None
        for l, blk in enumerate(t.h):
            x, delta, qkv = blk.forward_deferred_qkv(x, delta)
            # ragged: the cache rows len_b .. T0 - 1 of a shorter row come from pad columns here; each is
            # overwritten by the decode step that first reaches it (the append at p_b) before any read,
            # since a step at p_b reads rows <= p_b only
            D.cache_fill(qkv, self.cache, l, T0)
        # only the last prompt row goes through ln_f and the LM head: the [B * Tpad, Vp] logits are never formed
        if lens is None:
            xl, dl = x[:, T0 - 1].contiguous(), delta[:, T0 - 1].contiguous()
        else:                                    # row len_b - 1 of row b: a gather
            rows = torch.arange(B, device=dev)
            xl, dl = x[rows, ln - 1].contiguous(), delta[rows, ln - 1].contiguous()
        h = T.add_layer_norm_residual(xl, dl, t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
        self.state = D.DecodeState(dev, rng_state, pos=T0 - 1, step=0,
                                   row_offsets=None if lens is None else [n - T0 for n in lens])
        if lens is None:
            self.out = torch.zeros(B, T0 + n_new, device=dev, dtype=torch.int64)
            self.out[:, :T0] = idx
        else:
            self.out = torch.full((B, Tin + n_new), int(pad_token_id), device=dev, dtype=torch.int64)
            self.out[:, :Tin] = torch.where(real, idx, self.out[:, :Tin])
        self.next = torch.zeros(B, device=dev, dtype=torch.int64)
        self.logits_out = (torch.empty(B, n_new, self.V, device=dev, dtype=torch.bfloat16)
                           if return_logits else None)
        if self.processors is not None:          # allocated once; the prompt flags before the prefill's sample
            Vp = wte.shape[0]
            self.counts = D.TokenCounts(B, Vp, dev).add_prompt(idx, self.state, T0=T0)
            self.work = torch.empty(B, Vp, device=dev, dtype=torch.bfloat16)
            self.bias = self.processors.bias(B, self.V, Vp, dev)
            if self.history is not None:
                self.bias = self.history.merge_bias(self.bias, self.V, Vp, dev)
                if self.history.stop_sequences:
                    self.stop_hit = torch.full((B,), -1, device=dev, dtype=torch.int32)
        self._sample(D.skinny_linear(h, wte))      # token T0; the state now points at it

    def _sample(self, logits):
        temperature, top_k, eos, top_p = self.sampling
        if self.processors is not None:
            D.sample(logits, self.V, self.state, temperature, top_k, eos, next=self.next, out=self.out,
                     logits_out=self.logits_out, T0=self.T0, top_p=top_p, processors=self.processors,
                     counts=self.counts, processed_out=self.work, _bias=self.bias, history=self.history,
                     stop_hit=self.stop_hit)
            return
        D.sample(logits, self.V, self.state, temperature, top_k, eos, next=self.next, out=self.out,
                 logits_out=self.logits_out, T0=self.T0, top_p=top_p)

    def step(self):
        """embedding -> blocks (residual adds deferred into the next LayerNorm) -> ln_f -> LM head -> sampler"""
        t = self.model.transformer
        x, delta = D.decode_embed(self.next, t.wte.weight, t.wpe.weight, self.state), None
        for blk in t.h:
            x, delta = blk.decode_deferred(x, delta, self.cache, self.state)
        h = T.add_layer_norm_residual(x, delta, t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
        self._sample(D.skinny_linear(h, t.wte.weight))

    def capture(self):
        """The step as a graph.  An eager warm-up step runs first on a side stream and is undone by restoring
        the state it advanced (the cache row and output slot it wrote are written again, identically, by
        the first replay)."""
        dev = self.next.device
        saved = (self.state.buf.clone(), self.next.clone())
        counts = None if self.counts is None else self.counts.buf.clone()    # the warm-up step counts its token
        stop_hit = None if self.stop_hit is None else self.stop_hit.clone()  # ... and may stop a row
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self.step()
        cur.wait_stream(side)
        self.state.buf.copy_(saved[0])
        self.next.copy_(saved[1])
        if counts is not None:
            self.counts.buf.copy_(counts)
        if stop_hit is not None:
            self.stop_hit.copy_(stop_hit)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.step()
        return graph


def build_gpt2(cfg: GPTConfig = None, seed: int = 0, device=None, dtype=torch.bfloat16) -> GPT:
    torch.manual_seed(seed)
    m = GPT(cfg or GPTConfig())
    return m.to(device=device, dtype=dtype)
