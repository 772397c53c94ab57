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
