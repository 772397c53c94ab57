"""FP8 (OCP ``e4m3fn``) forward GEMMs for the GPT-2 block projections (``csrc/kernels/gemm_fp8.hip``).

The numeric definition, written once here; ``quantize_reference`` is its CPU twin and the GPU kernels match it
bit for bit:

* format ``torch.float8_e4m3fn`` (largest finite value 448);
* one scale per tensor, a power of two, from the tensor itself ("current scaling"): ``amax = max |t|`` in fp32,
  ``s = 2^k`` the largest power of two with ``amax * s <= 448``, ``k <= 126`` (so ``s`` and ``1 / s`` are normal
  fp32: only an ``amax`` below ``2^-118`` is affected), ``s = 1`` when ``amax == 0``;
* ``q = e4m3fn_rne(clamp(fp32(t) * s, -448, 448))`` -- the clamp is part of the definition (``torch``'s cast does
  not saturate); non-finite input is the caller's error, finite input never gives NaN;
* ``y[m, n] = bf16((sum_k float(xq[m, k]) float(wq[n, k])) * (1 / sx) * (1 / sw) + float(bias[n]))`` with fp32
  accumulation.  Every product of two e4m3 values is exact in fp32 and the scales are powers of two, so the only
  errors are the accumulation and the final rounding.  ``gelu=True`` writes ``gelu(pre)`` and ``gelu'(pre)`` of
  the bf16-rounded ``pre`` as ``gemm.fprop(gelu=True)`` does.

``Fp8Tensor(data, scale)``: ``data`` has the source's shape, ``scale`` is the fp32 block ``{s, 1 / s}``.  On the
GPU the block is written and read on the device only, so a captured step follows its data.

``quantize`` / ``quantize_many`` take contiguous bf16 GPU tensors whose last dimension is a multiple of 16
(``NotImplementedError`` otherwise): an amax launch and a cast launch, for the whole list at once.  They share a
small per-device workspace that the kernels re-arm themselves; it is created (zeroed) on the first call, which
must therefore happen outside a graph capture, and calls on one device must be ordered on one stream.

``linear_fp8`` / ``mlp_fp8``: the forward quantises the activations (and the weights, unless pre-quantised ones
are passed) and runs the FP8 GEMM; the backward is the bf16 op's (``LinearFn`` / ``MLPFn`` of
``ops/transformer.py``) on the saved bf16 operands, bit for bit.  CPU tensors run the twin: quantise, dequantise,
``F.linear`` in fp32, round to the input dtype, with straight-through gradients.

MXFP8 (``csrc/kernels/gemm_mxfp8.hip``, ``csrc/include/pde_mxfp8.h``): the same element format with one scale per
block of 32 consecutive elements of the last dimension, so that whoever holds a block can quantise it on the spot --
no amax pass over the tensor, no workspace, no atomics.  The definition; ``quantize_mx_reference`` is its CPU twin and
every GPU producer matches it bit for bit, sign of zero included:

* the last dimension is a multiple of 32; per block ``amax = max |t|`` in fp32; ``k = 0`` when ``amax == 0``, else
  with ``amax = m * 2^e``, ``m`` in ``[1, 2)``: ``k = 8 - e`` when ``m <= 1.75`` and ``7 - e`` otherwise, clamped to
  ``k <= 127`` -- the per-tensor rule above ("the largest power of two with ``amax * 2^k <= 448``") per block.  The
  OCP MX rule ``floor(log2 amax) - 8`` differs only for blocks with ``m > 1.75``: there OCP saturates the block's
  largest values at 448 and this rule does not;
* ``q = e4m3fn_rne(clamp(fp32(t) * 2^k, -448, 448))``; the scale byte is ``E = 127 - k`` (E8M0, in ``[0, 247]``,
  never 255) and the dequantised value is ``q * 2^(E - 127)``;
* ``y[m, n] = bf16(sum_g 2^(Ex[m, g] + Ew[n, g] - 254) (sum_{k in g} xq[m, k] wq[n, k]) + bias[n])``, fp32
  accumulation, one rounding; ``gelu=True`` as above.

``MxTensor(data, scale)``: ``data`` e4m3fn in the source's shape, ``scale`` uint8 ``[..., last / 32]``, contiguous.
``quantize_mx`` / ``quantize_mx_many`` (one launch for the whole list, capturable from the first call), ``fprop_mx``
(``K % 128 == 0``; ``act_mx=True`` with ``gelu`` also returns ``gelu(pre)`` as an ``MxTensor`` from the epilogue),
``linear_mx`` / ``mlp_mx`` (bf16 backward as above).  ``ops.transformer``'s LayerNorm ops produce an ``MxTensor`` of
their output with ``mx_out=True``.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch
import torch.nn.functional as F

from .._ext import kernels
from . import transformer as T

E4M3 = torch.float8_e4m3fn
E4M3_MAX = 448.0
MAX_K = 126
MX_BLOCK = 32
MX_MAX_K = 127


class Fp8Tensor(NamedTuple):
    data: torch.Tensor      # float8_e4m3fn, the source's shape
    scale: torch.Tensor     # fp32 [2]: {s, 1 / s}

    def dequantize(self) -> torch.Tensor:
        return self.data.float() * self.scale[1]


def quantize_reference(t: torch.Tensor) -> Fp8Tensor:
    """The definition above in plain torch, on the CPU: ``(q, scale)``."""
    x = t.detach().to("cpu", torch.float32)
    amax = x.abs().max() if x.numel() else torch.zeros(())
    mant, exp = torch.frexp(amax)                      # amax = mant * 2^exp, mant in [0.5, 1); 448 = 0.875 * 2^9
    k = torch.where(mant <= 0.875, 9 - exp, 8 - exp).clamp(max=MAX_K)
    k = torch.where(amax == 0, torch.zeros_like(k), k)
    s = torch.ldexp(torch.ones((), dtype=torch.float32), k)
    q = (x * s).clamp(-E4M3_MAX, E4M3_MAX).to(E4M3)
    return Fp8Tensor(q, torch.stack([s, 1.0 / s]))


_WORK = {}


def _work(device, n: int) -> torch.Tensor:
    w = _WORK.get(device)
    if w is None or w.numel() < 2 * n:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fp8.quantize: the first call on a device (or the first with a longer list) creates the "
                               "zeroed workspace and must run outside a graph capture")
        w = _WORK[device] = torch.zeros(2 * max(n, 64), device=device, dtype=torch.int32)
    return w


def quantize_many(tensors: Sequence[torch.Tensor]) -> List[Fp8Tensor]:
    """Quantise a list of bf16 GPU tensors with one amax launch and one cast launch (per 64 tensors)."""
    tensors = list(tensors)
    if not tensors:
        return []
    dev = tensors[0].device
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and t.dim() >= 1 and t.numel() > 0
                and t.shape[-1] % 16 == 0 and t.device == dev):
            raise NotImplementedError("fp8.quantize: contiguous bf16 GPU tensors on one device whose last dimension "
                                      f"is a multiple of 16 (got {tuple(t.shape)} {t.dtype} on {t.device})")
    flat = torch.empty(sum(t.numel() for t in tensors), device=dev, dtype=torch.uint8)
    scales = torch.empty(len(tensors), 2, device=dev, dtype=torch.float32)
    dst, off = [], 0
    for t in tensors:
        dst.append(flat[off:off + t.numel()])
        off += t.numel()
    kernels().fp8_quantize_many([t.detach() for t in tensors], dst, list(scales.unbind(0)), _work(dev, len(tensors)))
    return [Fp8Tensor(d.view(E4M3).view(t.shape), scales[i]) for i, (t, d) in enumerate(zip(tensors, dst))]


def quantize(t: torch.Tensor) -> Fp8Tensor:
    """``t`` (bf16, GPU) -> ``Fp8Tensor``; CPU tensors run ``quantize_reference``."""
    if not t.is_cuda:
        return quantize_reference(t)
    return quantize_many([t])[0]


def fprop(xq: Fp8Tensor, wq: Fp8Tensor, bias: Optional[torch.Tensor] = None, gelu: bool = False,
          out_dtype: torch.dtype = torch.bfloat16):
    """``xq`` [M, K] . ``wq`` [N, K]^T (+ bias) -> y [M, N]; with ``gelu`` returns ``(gelu(y), gelu'(y))``.  GPU: the
    FP8 MFMA GEMM (bf16 out, ``N % 8 == 0``, ``K % 64 == 0``).  CPU: the twin, rounded to ``out_dtype``."""
    M, K = xq.data.shape
    N = wq.data.shape[0]
    if xq.data.is_cuda:
        if N % 8 or K % 64 or wq.data.shape[1] != K:
            raise NotImplementedError(f"fp8.fprop: needs N % 8 == 0 and K % 64 == 0 (got M {M}, N {N}, K {K})")
        y = torch.empty(M, N, device=xq.data.device, dtype=torch.bfloat16)
        y2 = torch.empty_like(y) if gelu else None
        kernels().gemm_fp8(xq.data.view(torch.uint8), wq.data.view(torch.uint8), xq.scale, wq.scale, y, bias=bias, y2=y2)
        return (y, y2) if gelu else y
    pre = F.linear(xq.data.float(), wq.data.float()) * (xq.scale[1] * wq.scale[1])
    if bias is not None:
        pre = pre + bias.float()
    pre = pre.to(out_dtype)
    if not gelu:
        return pre
    p = pre.float().requires_grad_()
    with torch.enable_grad():
        act = F.gelu(p, approximate="tanh")
        (d,) = torch.autograd.grad(act.sum(), p)
    return act.detach().to(out_dtype), d.to(out_dtype)


def _wq(w, data, scale):
    return quantize(w) if data is None else Fp8Tensor(data, scale)


class LinearFp8Fn(T.LinearFn):
    """``LinearFn`` with the FP8 forward; the backward is ``LinearFn``'s on the saved bf16 ``x`` and ``w``."""

    @staticmethod
    def forward(ctx, x, w, b, wq_data, wq_scale):
        fin = w.shape[1]
        x2 = T._c(x.reshape(-1, fin))
        ctx.save_for_backward(x2, w)
        ctx.has_b = b is not None
        ctx.bias = b
        ctx.xshape = x.shape
        return fprop(quantize(x2), _wq(w, wq_data, wq_scale), b).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        return T.LinearFn.backward(ctx, dy) + (None, None)


class MLPFp8Fn(T.MLPFn):
    """``MLPFn`` with both forward GEMMs in FP8 (c_fc still writes gelu(pre) and gelu'(pre)); ``MLPFn``'s backward."""

    @staticmethod
    def forward(ctx, x, w_fc, b_fc, w_proj, b_proj, fc_data, fc_scale, proj_data, proj_scale):
        C = x.shape[-1]
        x2 = T._c(x.reshape(-1, C))
        act, dgelu = fprop(quantize(x2), _wq(w_fc, fc_data, fc_scale), b_fc, gelu=True)
        y = fprop(quantize(act), _wq(w_proj, proj_data, proj_scale), b_proj)
        ctx.save_for_backward(x2, w_fc, w_proj, dgelu, act)
        ctx.biases = (b_fc, b_proj)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], w_proj.shape[0])

    @staticmethod
    def backward(ctx, dy):
        return T.MLPFn.backward(ctx, dy) + (None, None, None, None)


class _CpuLinearFp8Fn(torch.autograd.Function):
    """The twin's forward with the gradients of ``F.linear`` on the unquantised operands (straight-through)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w, b)
        fin = w.shape[1]
        y = fprop(quantize_reference(x.reshape(-1, fin)), quantize_reference(w), b, out_dtype=x.dtype)
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        ins = [t.detach().requires_grad_(need) for t, need in zip((x, w, b), ctx.needs_input_grad) if t is not None]
        with torch.enable_grad():
            y = F.linear(*ins)
        want = [t for t in ins if t.requires_grad]
        grads = iter(torch.autograd.grad(y, want, dy) if want else ())
        out = [next(grads) if t.requires_grad else None for t in ins]
        return tuple(out) + (None,) * (3 - len(out))


def _check_gpu(name, x, weights):
    if x.dtype != torch.bfloat16 or any(w.dtype != torch.bfloat16 or w.shape[0] % 8 or w.shape[1] % 64 for w in weights):
        raise NotImplementedError(f"{name}: the GPU path is bf16 with out_features % 8 == 0 and in_features % 64 == 0 "
                                  f"(got x {x.dtype}, w {[tuple(w.shape) for w in weights]})")


def linear_fp8(x, w, b=None, wq: Optional[Fp8Tensor] = None):
    """``ops.transformer.linear`` with the FP8 forward.  ``wq``: ``w`` already quantised (``quantize_many``)."""
    if x.is_cuda:
        _check_gpu("linear_fp8", x, (w,))
        return LinearFp8Fn.apply(x, w, b, *(wq if wq is not None else (None, None)))
    return _CpuLinearFp8Fn.apply(x, w, b)


def mlp_fp8(x, w_fc, b_fc, w_proj, b_proj, wq_fc: Optional[Fp8Tensor] = None, wq_proj: Optional[Fp8Tensor] = None):
    """``ops.transformer.mlp`` with both forward GEMMs in FP8."""
    if x.is_cuda:
        _check_gpu("mlp_fp8", x, (w_fc, w_proj))
        for t in (b_fc, b_proj):
            if t.dtype != torch.bfloat16:
                raise NotImplementedError("mlp_fp8: the GPU path is bf16")
        return MLPFp8Fn.apply(x, w_fc, b_fc, w_proj, b_proj, *(wq_fc if wq_fc is not None else (None, None)),
                              *(wq_proj if wq_proj is not None else (None, None)))
    return linear_fp8(F.gelu(linear_fp8(x, w_fc, b_fc), approximate="tanh"), w_proj, b_proj)


# ------------------------------------------------------------------------------------------------ MXFP8
class MxTensor(NamedTuple):
    data: torch.Tensor      # float8_e4m3fn, the source's shape
    scale: torch.Tensor     # uint8 [..., last / 32]: E = 127 - k per block

    def dequantize(self) -> torch.Tensor:
        """fp32 ``q * 2^(E - 127)``, in plain torch on the CPU."""
        q = self.data.to("cpu").float().unflatten(-1, (-1, MX_BLOCK)).double()
        e = self.scale.to("cpu").double().unsqueeze(-1) - 127.0
        return (q * torch.pow(torch.full_like(e, 2.0), e)).flatten(-2).float()


def quantize_mx_reference(t: torch.Tensor) -> MxTensor:
    """The MX definition above in plain torch, on the CPU."""
    if t.dim() < 1 or t.shape[-1] % MX_BLOCK:
        raise ValueError(f"quantize_mx: the last dimension must be a multiple of {MX_BLOCK} (got {tuple(t.shape)})")
    x = t.detach().to("cpu", torch.float32).unflatten(-1, (-1, MX_BLOCK))
    amax = x.abs().amax(-1)
    mant, exp = torch.frexp(amax)                      # amax = mant * 2^exp, mant in [0.5, 1); 448 = 0.875 * 2^9
    k = torch.where(mant <= 0.875, 9 - exp, 8 - exp).clamp(max=MX_MAX_K)
    k = torch.where(amax == 0, torch.zeros_like(k), k)
    s = ((k + 127) << 23).to(torch.int32).view(torch.float32)       # 2^k, k in [-120, 127]: a normal fp32
    q = (x * s.unsqueeze(-1)).clamp(-E4M3_MAX, E4M3_MAX).to(E4M3)
    return MxTensor(q.flatten(-2), (127 - k).to(torch.uint8))


def _mx_empty(shape, dev):
    return MxTensor(torch.empty(shape, device=dev, dtype=torch.uint8).view(E4M3),
                    torch.empty(*shape[:-1], shape[-1] // MX_BLOCK, device=dev, dtype=torch.uint8))


def quantize_mx_many(tensors: Sequence[torch.Tensor]) -> List[MxTensor]:
    """Quantise a list of contiguous bf16 GPU tensors with one launch (per 64 tensors); CPU tensors run the
    reference."""
    tensors = list(tensors)
    if not tensors:
        return []
    if not tensors[0].is_cuda:
        return [quantize_mx_reference(t) for t in tensors]
    dev = tensors[0].device
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and t.dim() >= 1 and t.numel() > 0
                and t.shape[-1] % MX_BLOCK == 0 and t.device == dev):
            raise NotImplementedError("fp8.quantize_mx: contiguous bf16 GPU tensors on one device whose last dimension "
                                      f"is a multiple of 32 (got {tuple(t.shape)} {t.dtype} on {t.device})")
    n = sum(t.numel() for t in tensors)
    flat = torch.empty(n + n // MX_BLOCK, device=dev, dtype=torch.uint8)     # data first: every piece stays 16-byte aligned
    out, off, soff = [], 0, n
    for t in tensors:
        out.append(MxTensor(flat[off:off + t.numel()].view(E4M3).view(t.shape),
                            flat[soff:soff + t.numel() // MX_BLOCK].view(*t.shape[:-1], t.shape[-1] // MX_BLOCK)))
        off += t.numel()
        soff += t.numel() // MX_BLOCK
    kernels().mx_quantize_many([t.detach() for t in tensors], [q.data.view(torch.uint8) for q in out],
                               [q.scale for q in out])
    return out


def quantize_mx(t: torch.Tensor) -> MxTensor:
    """``t`` (bf16, GPU) -> ``MxTensor`` by ``k_mx_quant``; CPU tensors run ``quantize_mx_reference``."""
    return quantize_mx_many([t])[0]


def fprop_mx(xq: MxTensor, wq: MxTensor, bias: Optional[torch.Tensor] = None, gelu: bool = False, act_mx: bool = False,
             out_dtype: torch.dtype = torch.bfloat16):
    """``xq`` [M, K] . ``wq`` [N, K]^T (+ bias) -> y [M, N]; with ``gelu`` ``(gelu(y), gelu'(y))`` and with ``act_mx``
    as well ``(gelu(y), gelu'(y), quantize_mx(gelu(y)))``, the last written by the same launch.  GPU: the block-scaled
    MFMA GEMM (bf16 out, ``N % 8 == 0``, ``K % 128 == 0``, ``act_mx``: ``N % 32 == 0``).  CPU: the twin -- dequantise,
    ``F.linear`` in fp32, round to ``out_dtype``."""
    M, K = xq.data.shape
    N = wq.data.shape[0]
    if act_mx and not gelu:
        raise ValueError("fp8.fprop_mx: act_mx goes with gelu=True")
    if xq.data.is_cuda:
        if wq.data.shape[1] != K or K % 128 or N % 8 or (act_mx and N % MX_BLOCK):
            raise ValueError(f"fp8.fprop_mx: needs K % 128 == 0 and N % 8 == 0 (N % 32 == 0 with act_mx); got M {M}, "
                             f"N {N}, K {K}")
        y = torch.empty(M, N, device=xq.data.device, dtype=torch.bfloat16)
        y2 = torch.empty_like(y) if gelu else None
        aq = _mx_empty((M, N), y.device) if act_mx else MxTensor(None, None)
        kernels().gemm_mxfp8(xq.data.view(torch.uint8), wq.data.view(torch.uint8), xq.scale, wq.scale, y, bias=bias,
                             y2=y2, aq=None if aq.data is None else aq.data.view(torch.uint8), ae=aq.scale)
        return (y, y2, aq) if act_mx else (y, y2) if gelu else y
    pre = F.linear(xq.dequantize(), wq.dequantize())
    if bias is not None:
        pre = pre + bias.float()
    pre = pre.to(out_dtype)
    if not gelu:
        return pre
    p = pre.float().requires_grad_()
    with torch.enable_grad():
        act = F.gelu(p, approximate="tanh")
        (d,) = torch.autograd.grad(act.sum(), p)
    act = act.detach().to(out_dtype)
    return (act, d.to(out_dtype), quantize_mx_reference(act)) if act_mx else (act, d.to(out_dtype))


def _mx(t, data, scale):
    return quantize_mx(t) if data is None else MxTensor(data, scale)


def _pair(q):
    return tuple(q) if q is not None else (None, None)


class LinearMxFn(T.LinearFn):
    """``LinearFn`` with the MXFP8 forward; the backward is ``LinearFn``'s on the saved bf16 ``x`` and ``w``."""

    @staticmethod
    def forward(ctx, x, w, b, wq_data, wq_scale, xq_data, xq_scale):
        fin = w.shape[1]
        x2 = T._c(x.reshape(-1, fin))
        ctx.save_for_backward(x2, w)
        ctx.has_b = b is not None
        ctx.bias = b
        ctx.xshape = x.shape
        xq = quantize_mx(x2) if xq_data is None else MxTensor(xq_data.view(-1, fin), xq_scale.view(-1, fin // MX_BLOCK))
        return fprop_mx(xq, _mx(w, wq_data, wq_scale), b).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        return T.LinearFn.backward(ctx, dy) + (None, None, None, None)


class MLPMxFn(T.MLPFn):
    """``MLPFn`` with both forward GEMMs in MXFP8: c_fc writes gelu(pre), gelu'(pre) and, from the same epilogue, the
    ``MxTensor`` of gelu(pre) that c_proj reads; ``MLPFn``'s backward."""

    @staticmethod
    def forward(ctx, x, w_fc, b_fc, w_proj, b_proj, fc_data, fc_scale, proj_data, proj_scale, xq_data, xq_scale):
        C = x.shape[-1]
        x2 = T._c(x.reshape(-1, C))
        xq = quantize_mx(x2) if xq_data is None else MxTensor(xq_data.view(-1, C), xq_scale.view(-1, C // MX_BLOCK))
        act, dgelu, aq = fprop_mx(xq, _mx(w_fc, fc_data, fc_scale), b_fc, gelu=True, act_mx=True)
        y = fprop_mx(aq, _mx(w_proj, proj_data, proj_scale), b_proj)
        ctx.save_for_backward(x2, w_fc, w_proj, dgelu, act)
        ctx.biases = (b_fc, b_proj)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], w_proj.shape[0])

    @staticmethod
    def backward(ctx, dy):
        return T.MLPFn.backward(ctx, dy) + (None,) * 6


class _CpuLinearMxFn(_CpuLinearFp8Fn):
    """The MX twin's forward with ``_CpuLinearFp8Fn``'s straight-through gradients."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w, b)
        fin = w.shape[1]
        y = fprop_mx(quantize_mx_reference(x.reshape(-1, fin)), quantize_mx_reference(w), b, out_dtype=x.dtype)
        return y.view(*x.shape[:-1], w.shape[0])


def _check_gpu_mx(name, x, weights):
    if x.dtype != torch.bfloat16 or any(w.dtype != torch.bfloat16 or w.shape[0] % 32 or w.shape[1] % 128 for w in weights):
        raise NotImplementedError(f"{name}: the GPU path is bf16 with out_features % 32 == 0 and in_features % 128 == 0 "
                                  f"(got x {x.dtype}, w {[tuple(w.shape) for w in weights]})")


def linear_mx(x, w, b=None, wq: Optional[MxTensor] = None, xq: Optional[MxTensor] = None):
    """``ops.transformer.linear`` with the MXFP8 forward.  ``wq`` / ``xq``: ``w`` / ``x`` already quantised (by
    ``quantize_mx_many`` or by the kernel that produced ``x``)."""
    if x.is_cuda:
        _check_gpu_mx("linear_mx", x, (w,))
        return LinearMxFn.apply(x, w, b, *_pair(wq), *_pair(xq))
    return _CpuLinearMxFn.apply(x, w, b)


def mlp_mx(x, w_fc, b_fc, w_proj, b_proj, wq_fc: Optional[MxTensor] = None, wq_proj: Optional[MxTensor] = None,
           xq: Optional[MxTensor] = None):
    """``ops.transformer.mlp`` with both forward GEMMs in MXFP8."""
    if x.is_cuda:
        _check_gpu_mx("mlp_mx", x, (w_fc, w_proj))
        for t in (b_fc, b_proj):
            if t.dtype != torch.bfloat16:
                raise NotImplementedError("mlp_mx: the GPU path is bf16")
        return MLPMxFn.apply(x, w_fc, b_fc, w_proj, b_proj, *_pair(wq_fc), *_pair(wq_proj), *_pair(xq))
    return linear_mx(F.gelu(linear_mx(x, w_fc, b_fc), approximate="tanh"), w_proj, b_proj)
