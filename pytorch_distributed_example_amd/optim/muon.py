"""Muon for bf16 matrices with fp32 master weights: momentum SGD whose update is orthogonalised by a short
Newton-Schulz iteration in bf16 (``csrc/kernels/muon.hip``).  AdamW stays on embeddings, LayerNorm parameters and
biases: ``GPT.muon_groups()`` returns the split, and a ``MuonMaster`` runs beside an ``AdamWMaster`` over the rest.

The definition (the kernels implement it, ``ops.newton_schulz_reference`` is its CPU twin).  For a matrix parameter
``W [R, C]`` with bf16 weight, fp32 master ``Wm``, fp32 momentum buffer ``M``, bf16 gradient ``g`` already multiplied
by ``grad_scale``, and the fixed coefficients ``(a, b, c) = (3.4445, -4.7750, 2.0315)``::

    M  <- mu M + g                              U = g + mu M  (nesterov)  or  M
    X  <- bf16(U / (||U||_F + 1e-7))            in the wide orientation: n = min(R, C) rows, m = max(R, C) columns
    repeat ns_steps times:
        A <- bf16(X X^T)                        [n, n], fp32 accumulation, one rounding
        B <- bf16(b A + c (A A))                the axpy in fp32 in the epilogue, one rounding
        X <- bf16(a X + B X)                    likewise
    O  =  X back in W's orientation
    Wm <- Wm (1 - lr wd) - lr sqrt(max(1, R / C)) O          W <- bf16(Wm)

``||U||_F`` is reduced per matrix in a fixed order (one partial per 64 x 64 tile, folded in index order, no atomics),
so two runs and two replicas give the same bits.  ``lr`` comes from the attached table when there is one
(``set_lr_table``, as in ``AdamWMaster``); with ``capturable=True`` the step count is the device counter and the
whole step -- 2 prologue launches, 3 per iteration for all matrices together, 1 apply launch -- can be captured into
a hipGraph from its first call once the state exists (one eager step, or ``state_tensors()``).

Limits: every parameter 2-D bf16 on the GPU, both dimensions multiples of 64, below 2 GiB (``ValueError``).  The
optimizer owns a flat layout over exactly the matrices it is given; parameters already bound to a flat layout that
also holds other parameters (a DDP wrap of the whole model) are refused.
"""
from __future__ import annotations

import torch

from .._ext import kernels
from ..ops import muon as NS
from ..parallel.flat import shared_flat
from .master import _MasterBase


class MuonMaster(_MasterBase):
    _state_keys = ("momentum_buffer",)

    def __init__(self, params, lr=0.02, momentum=0.95, nesterov=True, ns_steps=5, weight_decay=0.0,
                 grad_scale: float = 1.0, capturable: bool = False):
        if not 0 <= int(ns_steps) <= 64:
            raise ValueError(f"MuonMaster: ns_steps must be in [0, 64], got {ns_steps}")
        super().__init__(params, dict(lr=lr, momentum=momentum, nesterov=nesterov, ns_steps=int(ns_steps),
                                      weight_decay=weight_decay), grad_scale)
        self.capturable = capturable
        for p in self._all_params():
            if p.dim() != 2:
                raise ValueError(f"MuonMaster: every parameter must be a 2-D matrix, got shape {tuple(p.shape)}")
            r, c = p.shape
            if r % 64 or c % 64 or r * c * 2 >= 1 << 31:
                raise ValueError("MuonMaster: matrix dimensions must be multiples of 64 and the matrix below 2 GiB, "
                                 f"got {r} x {c}")

    def _build(self):
        params = self._all_params()
        if any(getattr(p, "_pde_flat", None) is not None for p in params) and shared_flat(params) is None:
            raise RuntimeError("MuonMaster: its parameters are bound to a flat layout shared with other parameters "
                               "(wrapped in DDP as a whole?); it needs a layout over exactly its own matrices")
        super()._build()
        f = self._flat
        f["ws"] = NS.Workspace([tuple(p.shape) for p in params], f["p"].device)
        view = f["layout"].view
        names = [p._pde_flat[3] for p in params]
        f["mats"] = {k: [view(buf, n) for n in names]
                     for k, buf in (("p", f["p"]), ("g", f["g"]), ("master", f["bufs"]["master"]),
                                    ("mom", f["bufs"]["momentum_buffer"]))}
        f["wd"] = [float(g["weight_decay"]) for g in self.param_groups for _ in g["params"]]

    def _kernel(self):
        f, K = self._flat, kernels()
        g0, m, ws = self.param_groups[0], self._flat["mats"], self._flat["ws"]
        if self.capturable:
            f["step_dev"].add_(1.0)          # in stream order: a graph replay counts too
        K.muon_prologue(m["g"], m["mom"], ws.x, ws.partials, g0["momentum"], bool(g0["nesterov"]), self.grad_scale)
        res = ws.iterate(g0["ns_steps"])
        K.muon_apply(res, m["master"], m["p"], g0["lr"], f["wd"], step=self._step,
                     step_dev=f["step_dev"] if self.capturable else None, lr_table=self._lr_table)

    def load_state_dict(self, state_dict):
        if self._flat is None:
            self._build()                    # before the load: building afterwards would reset the loaded step count
        super().load_state_dict(state_dict)
        # torch casts loaded state to the parameters' dtype (bf16): put the fp32 values back, bit for bit
        f = self._flat
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        for i, p in zip(ids, self._all_params()):
            src = state_dict["state"].get(i, {})
            for k in f["bufs"]:
                if isinstance(src.get(k), torch.Tensor):
                    self.state[p][k].copy_(src[k])
        kernels().f32_to_bf16(f["bufs"]["master"], f["p"])
