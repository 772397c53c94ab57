"""Newton-Schulz orthogonalisation of bf16 matrices (``csrc/kernels/muon.hip``): Muon's hot path.

The numeric definition stands in ``optim/muon.py``.  ``newton_schulz_reference`` is its CPU twin: the same recurrence
in fp64 with a bf16 round-trip at exactly the definition's rounding points (``emulate=False``: the plain fp64
iteration).  ``newton_schulz`` runs a list of bf16 GPU matrices through the grouped HIP launches -- two prologue
launches, three GEMM launches per iteration for the whole list, one launch that writes the results back in each
matrix's own orientation -- and CPU tensors through the twin.  ``gram`` and ``apply_sym`` are the single stages.

Limits on the GPU (``ValueError``): 2-D contiguous bf16, both dimensions multiples of 64, each matrix below 2 GiB.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .._ext import kernels

NS_COEFFS = (3.4445, -4.7750, 2.0315)
NS_EPS = 1e-7


def _bf16_rt(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float64)


def newton_schulz_reference(x: torch.Tensor, steps: int = 5, emulate: bool = True) -> torch.Tensor:
    """The definition's ``X0 .. O`` on the CPU in fp64.  ``emulate=True`` rounds to bf16 where the kernels do (X0 and
    the three products of every iteration) and returns bf16; ``emulate=False`` rounds nowhere and returns fp64.  The
    input is taken as given (bf16 inputs are exact in fp64)."""
    a, b, c = NS_COEFFS
    rt = _bf16_rt if emulate else (lambda t: t)
    u = x.detach().to("cpu", torch.float64)
    tall = u.shape[0] > u.shape[1]
    if tall:
        u = u.t()
    X = rt(u / (u.norm() + NS_EPS))
    for _ in range(steps):
        A = rt(X @ X.t())
        B = rt(b * A + c * (A @ A))
        X = rt(a * X + B @ X)
    if tall:
        X = X.t()
    X = X.contiguous()
    return X.to(torch.bfloat16) if emulate else X


def check_matrices(xs: Sequence[torch.Tensor], what: str) -> None:
    if len(xs) == 0:
        raise ValueError(f"{what}: no matrices")
    for x in xs:
        if x.dim() != 2:
            raise ValueError(f"{what}: every matrix must be 2-D, got shape {tuple(x.shape)}")
        if x.dtype != torch.bfloat16:
            raise ValueError(f"{what}: bf16 matrices expected, got {x.dtype}")
        r, c = x.shape
        if r % 64 or c % 64 or r == 0 or c == 0 or r * c * 2 >= 1 << 31:
            raise ValueError(f"{what}: dimensions must be multiples of 64 and the matrix below 2 GiB, got {r} x {c}")
        if x.device != xs[0].device:
            raise ValueError(f"{what}: matrices on different devices")


class Workspace:
    """Scratch of the iteration for a fixed list of shapes: the wide ping-pong pair ``x`` / ``xalt`` [n, m], the
    [n, n] pair ``A`` / ``B`` and the norm partials, each kind in one allocation."""

    def __init__(self, shapes, device):
        wide = [(min(r, c), max(r, c)) for r, c in shapes]

        def carve(sizes):
            flat = torch.empty(sum(a * b for a, b in sizes), device=device, dtype=torch.bfloat16)
            out, o = [], 0
            for a, b in sizes:
                out.append(flat[o:o + a * b].view(a, b))
                o += a * b
            return out

        self.x, self.xalt = carve(wide), carve(wide)
        self.A, self.B = carve([(n, n) for n, _ in wide]), carve([(n, n) for n, _ in wide])
        self.partials = torch.empty(sum((r // 64) * (c // 64) for r, c in shapes), device=device, dtype=torch.float32)

    def iterate(self, steps: int):
        """Run the iteration on ``self.x``; returns the list that holds the result."""
        a, b, c = NS_COEFFS
        return self.xalt if kernels().muon_ns(self.x, self.xalt, self.A, self.B, steps, a, b, c) else self.x


def newton_schulz(xs: Sequence[torch.Tensor], steps: int = 5) -> List[torch.Tensor]:
    """Orthogonalise every matrix of ``xs`` (the definition's ``X0 .. O`` with ``U = x``); returns new bf16 tensors."""
    xs = list(xs)
    if not xs:
        raise ValueError("newton_schulz: no matrices")
    if not xs[0].is_cuda:
        return [newton_schulz_reference(x, steps) for x in xs]
    check_matrices(xs, "newton_schulz")
    xs = [x.contiguous() for x in xs]
    K = kernels()
    ws = Workspace([tuple(x.shape) for x in xs], xs[0].device)
    K.muon_prologue(xs, None, ws.x, ws.partials, 0.0, False, 1.0)
    res = ws.iterate(steps)
    out = [torch.empty_like(x) for x in xs]
    K.muon_apply(res, None, out, 0.0, [0.0] * len(xs))
    return out


def gram(ps: Sequence[torch.Tensor], cs: Optional[Sequence[torch.Tensor]] = None, alpha: float = 0.0,
         beta: float = 1.0) -> List[torch.Tensor]:
    """One symmetric stage for the whole list in one launch: ``bf16(alpha c + beta p p^T)`` with ``c`` symmetric
    [n, n] (absent: ``bf16(beta p p^T)``).  Only the upper tiles are computed; the result is symmetric bit for bit."""
    ps = list(ps)
    check_matrices(ps, "gram")
    out = [torch.empty(p.shape[0], p.shape[0], device=p.device, dtype=torch.bfloat16) for p in ps]
    kernels().muon_gemm_sym(ps, None if cs is None else list(cs), out, alpha, beta)
    return out


def apply_sym(bs: Sequence[torch.Tensor], xs: Sequence[torch.Tensor], alpha: float) -> List[torch.Tensor]:
    """The rectangular stage in one launch: ``bf16(alpha x + b x)`` for symmetric ``b`` [n, n] and ``x`` [n, m]."""
    bs, xs = list(bs), list(xs)
    check_matrices(xs, "apply_sym")
    out = [torch.empty_like(x) for x in xs]
    kernels().muon_gemm_rect(bs, xs, xs, out, alpha, 1.0)
    return out
