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

    def decode_deferred(self, x, delta, cache, state, beam_table=None):
        """One-token ``forward_deferred`` over the decode kernels: ``x`` / ``delta`` are ``[B, C]``, the
        new K and V are appended to ``cache`` at the position held by ``state``.  ``beam_table`` (a beam search's
        ancestor table) makes the attention read the earlier positions through it."""
        if delta is None:
            x, h = T.layer_norm_residual(x, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        else:
            x, h = T.add_layer_norm_residual(x, delta, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        qkv = D.skinny_linear(h, self.attn.c_attn.weight, self.attn.c_attn.bias)
        if beam_table is None:
            a = D.decode_attention(qkv, cache, self.layer_idx, state)
        else:
            a = D.decode_attention(qkv, cache, self.layer_idx, state, beam_table=beam_table)
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
                 no_repeat_ngram_size=0, bad_words_ids=None, stop_sequences=None, num_beams=1, length_penalty=1.0,
                 return_beams=False, _beam_trace=None):
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

        ``num_beams = K > 1`` runs beam search instead of sampling (definition in ``ops/decode.py``): every prompt
        keeps ``K`` hypotheses, every step extends them by the ``K`` best of their continuations by cumulative
        log-probability, a hypothesis that emits ``eos_token_id`` is frozen, and after ``max_new_tokens`` steps they
        are ranked by ``score / length ** length_penalty``.  The result is the best hypothesis per prompt in the
        layout above; ``return_beams=True`` returns ``(out [B, K, T0 + max_new_tokens], scores [B, K] fp32)`` in rank
        order instead, and ``return_logits`` adds the raw logits every physical row ``b * K + k`` saw,
        ``[B * K, max_new_tokens, V]`` by row and step (step 0 fills row ``b * K`` only).  It is deterministic: no
        random number is drawn and ``generator`` is not touched.  The sampling keywords, the processors and the
        history constraints must stay at their defaults with it (``ValueError``).  On the GPU ``B * K <= 16``; the
        prompt is prefilled once per prompt, the KV cache is never reordered -- the decode attention reads it
        through a small per-row ancestor table that the selection kernels rewrite -- and the selection runs on the
        device, so the step still replays as one graph.  With ``num_beams=1`` nothing changes and nothing is
        allocated.

        ``T0 + max_new_tokens`` (``max(prompt_lens) + max_new_tokens`` for a ragged batch) must not exceed
        ``block_size`` (learned absolute positions: no sliding window)."""
        cfg = self.config
        if idx.dim() != 2 or idx.shape[1] < 1:
            raise ValueError("generate: idx must be [B, T0] with T0 >= 1")
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be >= 1")
        if not 0 <= int(pad_token_id) < cfg.vocab_size:
            raise ValueError("generate: pad_token_id must be a token of the vocabulary")
        dev = self.transformer.wte.weight.device
        # num_beams and length_penalty are checked for every call; eos_token_id only where beam search runs, so the
        # sampling path keeps validating it where and as it did
        beam = D.BeamConfig(num_beams, length_penalty, who="generate")
        if return_beams and not beam.active:
            raise ValueError("generate: return_beams needs num_beams > 1")
        if beam.active:
            beam = D.BeamConfig(num_beams, length_penalty, eos_token_id, who="generate")
            given = dict(temperature=temperature != 1.0, top_k=top_k is not None, top_p=top_p is not None,
                         seed=seed is not None, generator=generator is not None,
                         repetition_penalty=repetition_penalty != 1.0, frequency_penalty=frequency_penalty != 0.0,
                         presence_penalty=presence_penalty != 0.0, logit_bias=logit_bias is not None,
                         suppress_tokens=suppress_tokens is not None, min_new_tokens=min_new_tokens != 0,
                         no_repeat_ngram_size=no_repeat_ngram_size != 0, bad_words_ids=bad_words_ids is not None,
                         stop_sequences=stop_sequences is not None)
            off = [name for name, on in given.items() if on]
            if off:
                raise ValueError(f"generate: num_beams > 1 does not combine with {', '.join(off)} (beam search is "
                                 "deterministic and takes no processors or constraints)")
            return self._generate_beam(idx.to(dev).long(), max_new_tokens, beam, prompt_lens, int(pad_token_id),
                                       return_logits, return_beams, use_graph, _after_prefill, _beam_trace)
        config = D.SamplerConfig(
            temperature, top_k, top_p, eos_token_id,
            D.LogitProcessors(repetition_penalty, frequency_penalty, presence_penalty, logit_bias, suppress_tokens,
                              min_new_tokens, eos_token_id),
            D.HistoryConstraints(no_repeat_ngram_size, bad_words_ids, stop_sequences, eos_token_id),
            who="generate")
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
                args = (idx.to(dev).long(), max_new_tokens, config, generator, prompt_lens, int(pad_token_id),
                        return_logits)
                if dev.type == "cuda":
                    return self._generate_gpu(*args, use_graph, _after_prefill)
                return self._generate_cpu(*args)
        finally:
            self.train(was_training)

    def _generate_beam(self, idx, n_new, beam, lens, pad, return_logits, return_beams, use_graph, _after_prefill,
                       trace):
        """``generate`` with ``num_beams > 1`` on either device.  ``trace`` (a dict, for tests) receives what every
        step chose -- ``tok``, ``parent``, ``score`` (``[n_new, B * K]``; on the CPU also ``gap``, ``[n_new, B]``, of
        ``beam_step_reference``) -- and the rows' final ``S``, ``len`` and ``finished``."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                if idx.is_cuda:
                    out, scores, logits, tr = self._generate_beam_gpu(idx, n_new, beam, lens, pad, return_logits,
                                                                      use_graph, _after_prefill)
                else:
                    out, scores, logits, tr = self._generate_beam_cpu(idx, n_new, beam, lens, pad, return_logits)
        finally:
            self.train(was_training)
        if trace is not None:
            trace.update(tr)
        res = (out, scores) if return_beams else (out[:, 0].contiguous(),)
        res = res + (logits,) if return_logits else res
        return res if len(res) > 1 else res[0]

    def _generate_beam_cpu(self, idx, n_new, beam, lens, pad, return_logits):
        """The plain definition: ``B * K`` hypotheses, a full forward per token, ``beam_step_reference``'s rule.  The
        hypotheses are reordered physically, so row ``b * K + j`` always holds beam ``j``'s tokens."""
        V, K = self.config.vocab_size, beam.num_beams
        B, Tin = idx.shape
        lens, Tl = _prompt_window(self.config, idx, n_new, lens, beam)
        R = B * K
        ln = torch.tensor(lens or [Tin] * B, dtype=torch.int64).repeat_interleave(K)
        rows, grp = torch.arange(R), (torch.arange(B) * K)[:, None]
        prompts = D._prompt_out(idx, lens, n_new, pad, "cpu")
        seq = torch.zeros(R, Tl + n_new, dtype=torch.int64)        # what the model sees: pad columns hold token 0
        seq[:, :Tl] = torch.where(torch.arange(Tl)[None, :] < ln[:, None], idx[:, :Tl].repeat_interleave(K, 0), 0)
        S, fin, length = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.bool), torch.zeros(
            R, dtype=torch.int64)
        tr = {k: [] for k in ("tok", "parent", "score", "gap")}
        logits_out = None
        for s in range(n_new):
            logits = self(seq[:, :Tl + s])[rows, ln + s - 1]
            if return_logits:
                if logits_out is None:
                    logits_out = torch.zeros(R, n_new, V, dtype=logits.dtype)
                logits_out[:, s] = logits[:, :V]
                if s == 0:
                    logits_out[(rows % K) != 0, 0] = 0
            parent, tok, score, info = D.beam_step_reference(logits, V, K, S, fin, beam.eos_token_id, first=s == 0,
                                                             return_info=True)
            src, tok = (grp + parent).reshape(R), tok.reshape(R)
            seq = seq[src]
            seq[rows, ln + s] = tok
            length = length[src] + (~fin[src]).long()
            fin = fin[src] | (tok == beam._eos)
            S = score.reshape(R)
            for k, v in (("tok", tok), ("parent", parent.reshape(R)), ("score", S), ("gap", torch.from_numpy(info["gap"]))):
                tr[k].append(v.clone())
        order, ranked = D.beam_rank_reference(S, length, K, beam.length_penalty)
        out = prompts[:, None, :].repeat(1, K, 1)
        for b in range(B):
            for i in range(K):
                r, n = b * K + int(order[b, i]), int(ln[b * K])
                out[b, i, n:n + n_new] = seq[r, n:n + n_new]
        tr = {k: torch.stack(v) for k, v in tr.items()}
        tr.update(S=S, len=length, finished=fin)
        return out, ranked.float(), logits_out, tr

    def _generate_beam_gpu(self, idx, n_new, beam, lens, pad, return_logits, use_graph, _after_prefill):
        ses = DecodeSession(self, idx, n_new, return_logits=return_logits, prompt_lens=lens, pad_token_id=pad, beam=beam)
        if _after_prefill is not None:
            _after_prefill(ses.cache)
        if n_new > 1 and use_graph:
            graph = ses.capture()
            for _ in range(n_new - 1):
                graph.replay()
        else:
            for _ in range(n_new - 1):
                ses.step()
        bb = ses.beam
        out, scores = bb.finalize()
        R = bb.B * bb.K
        tr = dict(tok=bb.tok, parent=bb.parent, score=bb.score_trace, S=bb.score, len=bb.len,
                  finished=bb.state.finished[:R])
        return out, scores, bb.logits_out, tr

    def _generate_cpu(self, idx, n_new, config, generator, lens, pad, return_logits):
        """One right-padded forward per token; row ``b``'s logits are row ``len_b + s - 1`` of it (causal:
        independent of what follows), gathered into ``[B, V]`` for one sampler call per step, so the
        Philox row index is ``b`` as on the GPU.  A batch of one prompt length is the ragged one with every
        ``len_b = T0``; the sampler's CPU twin keeps eos, the output layout and the draw number."""
        V = self.config.vocab_size
        B, T0 = idx.shape
        lens, Tl = _prompt_window(self.config, idx, n_new, lens, config)
        buf = D.SampleBuffers(config, idx, lens, n_new, V, V, "cpu", generator.state, pad, return_logits,
                              dtype=self.transformer.wte.weight.dtype)
        ln = torch.tensor(lens or [T0] * B, dtype=torch.int64)
        rows = torch.arange(B)
        seq = torch.zeros(B, Tl + n_new, dtype=torch.int64)        # what the model sees: pad columns hold token 0
        seq[:, :Tl] = torch.where(torch.arange(Tl)[None, :] < ln[:, None], idx[:, :Tl], seq[:, :Tl])
        for s in range(n_new):
            seq[rows, ln + s] = buf.sample(self(seq[:, :Tl + s])[rows, ln + s - 1])
        generator.state.copy_(buf.state.rng)       # the draw number advanced by n_new
        return (buf.out, buf.logits_out) if return_logits else buf.out

    def _generate_gpu(self, idx, n_new, config, generator, lens, pad, return_logits, use_graph, _after_prefill):
        ses = DecodeSession(self, idx, n_new, rng_state=generator.state, return_logits=return_logits, prompt_lens=lens,
                            pad_token_id=pad, config=config)
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


def _prompt_window(cfg, idx, n_new, prompt_lens, config):
    """``(lens, T0)`` of a generation of ``n_new`` tokens after ``idx``: the prompt lengths as a list (``None`` for a
    batch of one length) and the longest of them, checked against the width of ``idx`` and ``block_size``; and the
    checks of ``config`` (the ``ops.SamplerConfig``) against the batch, the vocabulary and the device."""
    B, Tin = idx.shape
    config.check(B, cfg.vocab_size, idx.device)
    lens = None
    if prompt_lens is not None:
        lens = D._int_list(prompt_lens)
        if len(lens) != B:
            raise ValueError(f"generate: prompt_lens holds {len(lens)} lengths for {B} rows")
        if min(lens) < 1 or max(lens) > Tin:
            raise ValueError(f"generate: every prompt length must be in 1 .. {Tin} (got {lens})")
    T0 = Tin if lens is None else max(lens)       # the longest prompt: window, cache length and base position
    if T0 + n_new > cfg.block_size:
        raise ValueError(f"generate: T0 + max_new_tokens = {T0 + n_new} exceeds block_size "
                         f"{cfg.block_size} (positions are learned and absolute: no sliding window)")
    return lens, T0


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
    included.  When none is on, ``history`` and ``stop_hit`` stay ``None``.

    ``config`` (an ``ops.SamplerConfig``, as ``GPT.generate`` passes) stands for all the sampling keywords.  The
    buffers named above live in ``buffers``, an ``ops.SampleBuffers``, and are mirrored as attributes.

    ``beam`` (an ``ops.BeamConfig`` with ``num_beams = K > 1``) makes it a beam search over ``B * K <= 16`` physical rows:
    the prefill still runs ``B`` rows and stores each prompt's K and V once, ``buffers`` is an ``ops.BeamBuffers`` (also
    ``beam``; ``None`` otherwise), every step's attention reads the cache through its ancestor table and the beam
    selection takes the sampler's place.  ``beam.finalize()`` ranks the hypotheses after the last step."""

    def __init__(self, model, idx, n_new, temperature=1.0, top_k=None, rng_state=None, eos=None,
                 return_logits=False, top_p=None, prompt_lens=None, pad_token_id=0, processors=None,
                 repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None,
                 suppress_tokens=None, min_new_tokens=0, history=None, no_repeat_ngram_size=0, bad_words_ids=None,
                 stop_sequences=None, config=None, beam=None):
        cfg, t = model.config, model.transformer
        dev = idx.device
        B = idx.shape[0]
        beam = beam if beam is not None and beam.active else None
        K = 1 if beam is None else beam.num_beams
        if beam is not None:
            config = beam               # the sampler's settings play no part; `check` has the same signature
        elif config is None:
            if processors is None:
                processors = D.LogitProcessors(repetition_penalty, frequency_penalty, presence_penalty, logit_bias,
                                               suppress_tokens, min_new_tokens, eos)
            if history is None:
                history = D.HistoryConstraints(no_repeat_ngram_size, bad_words_ids, stop_sequences, eos)
            config = D.SamplerConfig(temperature, top_k, top_p, eos, processors, history, who="generate")
        lens, T0 = _prompt_window(cfg, idx, n_new, prompt_lens, config)
        wte, wpe = t.wte.weight, t.wpe.weight
        if B * K > D.MAX_ROWS:
            raise NotImplementedError(f"generate: at most {D.MAX_ROWS} sequences on the GPU (got {B}"
                                      + (f" x {K} beams)" if K > 1 else ")"))
        if wte.dtype != torch.bfloat16:
            raise NotImplementedError("generate: the GPU path is bf16")
        Tpad = min(-(-T0 // 128) * 128, cfg.block_size)
        if Tpad % 128:
            raise NotImplementedError("generate: the prefill needs a window that is a multiple of 128 "
                                      f"(block_size {cfg.block_size} caps it at {Tpad})")
        self.model, self.T0, self.V = model, T0, cfg.vocab_size
        # prefill: the training kernels over the padded prompt (causal: the pad never reaches positions < T0)
        self.cache = D.KVCache(cfg, B * K, T0 + n_new, dev)
        idx_pad = torch.zeros(B, Tpad, device=dev, dtype=torch.int64)
        if lens is None:
            idx_pad[:, :T0] = idx
        else:                                    # columns >= len_b hold token 0, whatever idx holds there
            ln = torch.tensor(lens, device=dev, dtype=torch.int64)
            real = torch.arange(T0, device=dev)[None, :] < ln[:, None]
            idx_pad[:, :T0] = torch.where(real, idx[:, :T0], idx_pad[:, :T0])
        x, delta = T.embedding(idx_pad, wte, wpe), None
        for l, blk in enumerate(t.h):
            x, delta, qkv = blk.forward_deferred_qkv(x, delta)
            # ragged: the cache rows len_b .. T0 - 1 of a shorter row come from pad columns here; each is
            # overwritten by the decode step that first reaches it (the append at p_b) before any read,
            # since a step at p_b reads rows <= p_b only
            if beam is None:
                D.cache_fill(qkv, self.cache, l, T0)
            else:                                # once per prompt, into the group's first row
                D.cache_fill(qkv, self.cache, l, T0, num_beams=K)
        # only the last prompt row goes through ln_f and the LM head: the [B * Tpad, Vp] logits are never formed
        if lens is None:
            xl, dl = x[:, T0 - 1].contiguous(), delta[:, T0 - 1].contiguous()
        else:                                    # row len_b - 1 of row b: a gather
            rows = torch.arange(B, device=dev)
            xl, dl = x[rows, ln - 1].contiguous(), delta[rows, ln - 1].contiguous()
        h = T.add_layer_norm_residual(xl, dl, t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
        # state, next, out and logits_out; with processors or constraints on also counts (the prompt flags set), work,
        # bias and stop_hit, which stay None otherwise: the sampler is then called exactly as without them
        self.beam = self._table = None
        if beam is not None:
            # the B * K rows' state, scores, lengths, ancestor table and traces; the prompt's logits go to row b * K,
            # the only one the first beam step reads
            self.buffers = self.beam = b = D.BeamBuffers(beam, idx, lens, n_new, self.V, wte.shape[0], dev,
                                                         self.cache.max_len, pad_token_id, return_logits)
            self._table = b.table
            self.processors = self.history = self.counts = self.work = self.bias = self.stop_hit = None
            self.state, self.next, self.out, self.logits_out = b.state, b.next, b.out, b.logits_out
            logits = torch.zeros(B * K, wte.shape[0], device=dev, dtype=wte.dtype)
            logits[::K] = D.skinny_linear(h, wte)
            self._sample(logits)
            return
        self.buffers = b = D.SampleBuffers(config, idx, lens, n_new, self.V, wte.shape[0], dev, rng_state, pad_token_id,
                                           return_logits)
        self.processors, self.history = config.processors, config.history
        self.state, self.next, self.out, self.logits_out = b.state, b.next, b.out, b.logits_out
        self.counts, self.work, self.bias, self.stop_hit = b.counts, b.work, b.bias, b.stop_hit
        self._sample(D.skinny_linear(h, wte))      # token T0; the state now points at it

    def _sample(self, logits):
        self.buffers.sample(logits)

    def step(self):
        """embedding -> blocks (residual adds deferred into the next LayerNorm) -> ln_f -> LM head -> sampler"""
        t = self.model.transformer
        x, delta = D.decode_embed(self.next, t.wte.weight, t.wpe.weight, self.state), None
        for blk in t.h:
            x, delta = blk.decode_deferred(x, delta, self.cache, self.state, self._table)
        h = T.add_layer_norm_residual(x, delta, t.ln_f.weight, t.ln_f.bias, t.ln_f.eps)[1]
        self._sample(D.skinny_linear(h, t.wte.weight))

    def capture(self):
        """The step as a graph.  An eager warm-up step runs first on a side stream and is undone by restoring
        the state it advanced (the cache row and output slot it wrote are written again, identically, by
        the first replay)."""
        dev = self.next.device
        saved = self.buffers.snapshot()           # the warm-up step advances the state, counts its token, may stop a row
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self.step()
        cur.wait_stream(side)
        self.buffers.restore(saved)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.step()
        return graph


def build_gpt2(cfg: GPTConfig = None, seed: int = 0, device=None, dtype=torch.bfloat16) -> GPT:
    torch.manual_seed(seed)
    m = GPT(cfg or GPTConfig())
    return m.to(device=device, dtype=dtype)
