"""Learning-rate schedules that survive hipGraph replay.

A captured kernel launch freezes its by-value arguments, so a learning rate passed by value is fixed
for the life of a graph.  A schedule here is a device table of one fp32 rate per optimizer step; the
optimizer kernels index it with the step count they already keep on the device (step ``t``, 1-based,
uses ``table[min(t-1, len-1)]``: a run longer than the table keeps its last rate).  A table is exact
for any schedule, so every ``torch.optim.lr_scheduler`` class is usable through ``from_torch``.

``LRTable(target, lrs)`` is the scheduler object; ``target`` is one of the package's optimizers
(``optim.Adam`` / ``AdamW`` / ``SGD`` / ``AdamWMaster`` / ``SGDMaster``) or a ``LeNetTrainStep`` engine.
While a table is attached the GPU kernels take their rate from it and ignore ``group["lr"]``;
``step()`` still writes ``param_groups[i]["lr"]``, which is what CPU parameter groups and logging read.

Builders (lists of Python floats, the ``lrs`` argument; with ``target=`` they return an ``LRTable``):
``warmup_cosine`` -- entry k (optimizer step k+1) is ``base_lr*(k+1)/warmup_steps`` while
k < warmup_steps (first entry ``base_lr/warmup_steps``, never 0; the peak ``base_lr`` is the rate of
optimizer step ``warmup_steps``), then ``min_lr + (base_lr-min_lr)/2 * (1 + cos(pi*progress))`` with
progress reaching 1 (rate ``min_lr``) at the last entry; ``step_decay`` (``StepLR``) and ``constant``.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence

import torch


def make_table(lrs, device) -> torch.Tensor:
    """The fp32 device table of ``lrs``: every Python float is rounded to fp32 exactly as the kernels'
    by-value ``(float)lr`` argument cast rounds it (double -> float, round to nearest even)."""
    if isinstance(lrs, torch.Tensor):
        t = lrs.detach()
        if t.dtype != torch.float32:
            t = t.to(torch.float64).to(torch.float32)
    else:
        t = torch.tensor([float(x) for x in lrs], dtype=torch.float64).to(torch.float32)
    if t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"a learning-rate table needs a 1-D sequence of at least one rate, got shape {tuple(t.shape)}")
    return t.to(device).contiguous()


def check_table(table, device, what: str = "lr table") -> torch.Tensor:
    """Validate a table handed to ``set_lr_table``: a 1-D, non-empty fp32 tensor on ``device``."""
    if not isinstance(table, torch.Tensor):
        raise TypeError(f"{what}: a torch.Tensor is expected, got {type(table).__name__}")
    if table.dtype != torch.float32:
        raise TypeError(f"{what}: dtype {table.dtype}, expected torch.float32")
    if table.dim() != 1 or table.numel() < 1:
        raise ValueError(f"{what}: a 1-D table of at least one rate is expected, got shape {tuple(table.shape)}")
    if table.device != torch.device(device):
        raise ValueError(f"{what}: the table is on {table.device}, the parameters are on {device}")
    return table.contiguous()


def per_group_tables(tables, ngroups: int, devices, what: str):
    """Normalise ``set_lr_table``'s argument (None, one shared table, or one per group) to a list."""
    if tables is None:
        return [None] * ngroups
    if isinstance(tables, torch.Tensor):
        tables = [tables] * ngroups
    tables = list(tables)
    if len(tables) != ngroups:
        raise ValueError(f"{what}: {len(tables)} learning-rate tables for {ngroups} parameter groups")
    return [check_table(t, d, what) for t, d in zip(tables, devices)]


def _is_number(x) -> bool:
    return isinstance(x, (int, float)) or (isinstance(x, torch.Tensor) and x.dim() == 0)


class LRTable:
    """Table-driven learning-rate scheduler with the ``torch.optim.lr_scheduler`` surface."""

    def __init__(self, target, lrs):
        self.target = target
        self.optimizer = target                      # torch's attribute name
        groups = getattr(target, "param_groups", None)
        ngroups = len(groups) if groups is not None else 1
        shared = isinstance(lrs, torch.Tensor) and lrs.dim() == 1
        if not isinstance(lrs, torch.Tensor):
            lrs = list(lrs)
            if not lrs:
                raise ValueError("LRTable: an empty learning-rate list")
            shared = _is_number(lrs[0])
        per_group = [lrs] * ngroups if shared else list(lrs)
        if len(per_group) != ngroups:
            raise ValueError(f"LRTable: {len(per_group)} learning-rate lists for {ngroups} parameter groups")
        self._devices = self._group_devices()
        self._host = [make_table(x, "cpu") for x in ([per_group[0]] if shared else per_group)]
        if shared:
            self._host = self._host * ngroups
        self.last_epoch = 0
        self._attach()
        self._write_groups()

    # ------------------------------------------------------------------ plumbing
    def _group_devices(self):
        groups = getattr(self.target, "param_groups", None)
        if groups is None:
            return [self.target.device]
        return [g["params"][0].device for g in groups]

    def _attach(self):
        up = {}
        tabs = []
        for h, d in zip(self._host, self._devices):
            key = (id(h), str(d))
            if key not in up:                        # a shared table is uploaded once per device
                up[key] = h.to(d)
            tabs.append(up[key])
        self.tables = tabs
        if getattr(self.target, "param_groups", None) is None:
            self.target.set_lr_table(tabs[0])
        else:
            self.target.set_lr_table(tabs)

    def _sync(self) -> int:
        """The host's view never lags the device: optimizer steps taken inside graph replays count."""
        fn = getattr(self.target, "lr_step_count", None)
        n = fn() if fn is not None else None
        if n is not None and n > self.last_epoch:
            self.last_epoch = int(n)
        return self.last_epoch

    def lr_at(self, k: int) -> List[float]:
        """Entry ``k`` (0-based, clamped to the table) of every group: the rate of optimizer step k+1."""
        return [float(h[min(max(int(k), 0), h.numel() - 1)]) for h in self._host]

    def _write_groups(self):
        groups = getattr(self.target, "param_groups", None)
        if groups is not None:
            for g, lr in zip(groups, self.lr_at(self.last_epoch)):
                g["lr"] = lr

    # ------------------------------------------------------------------ torch scheduler surface
    def step(self, steps: int = 1):
        """Advance the host's view by ``steps`` optimizer steps and write ``param_groups[i]["lr"]``."""
        self.last_epoch += int(steps)
        self._write_groups()

    def get_last_lr(self) -> List[float]:
        """The rate the next optimizer step uses, from the optimizer's / engine's own step count (a
        host sync when that count lives on the device: a logging call)."""
        return self.lr_at(self._sync())

    def state_dict(self):
        return {"last_epoch": int(self.last_epoch), "tables": [h.clone() for h in self._host]}

    def load_state_dict(self, sd):
        tabs = sd.get("tables")
        if tabs is not None:
            if len(tabs) != len(self._host):
                raise ValueError(f"LRTable: state has {len(tabs)} tables, the scheduler {len(self._host)}")
            new = [make_table(t, "cpu") for t in tabs]
            if any(a.shape != b.shape or not torch.equal(a, b) for a, b in zip(new, self._host)):
                self._host = new
                self._attach()
        self.last_epoch = int(sd["last_epoch"])
        self._write_groups()


def from_torch(target, factory: Callable, num_steps: int) -> LRTable:
    """Tabulate any ``torch.optim.lr_scheduler``: ``factory(dummy_optimizer)`` is stepped ``num_steps``
    times on the CPU and ``get_last_lr()`` is recorded before each step, so entry k is the rate torch
    would use for optimizer step k+1."""
    groups = getattr(target, "param_groups", None)
    base = [float(g["lr"]) for g in groups] if groups is not None else [float(target.lr)]
    dummy = torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": lr} for lr in base], lr=base[0])
    sched = factory(dummy)
    rows = [[] for _ in base]
    for _ in range(int(num_steps)):
        for row, lr in zip(rows, sched.get_last_lr()):
            row.append(float(lr))
        dummy.step()
        sched.step()
    return LRTable(target, rows)


def _built(lrs, target):
    return lrs if target is None else LRTable(target, lrs)


def warmup_cosine(base_lr: float, warmup_steps: int, total_steps: int, min_lr: float = 0.0, target=None):
    """Linear warm-up to ``base_lr`` over ``warmup_steps`` steps, cosine decay to ``min_lr`` at step
    ``total_steps`` (see the module docstring for the exact entries)."""
    if total_steps < 1 or warmup_steps < 0 or warmup_steps > total_steps:
        raise ValueError("warmup_cosine: need 0 <= warmup_steps <= total_steps and total_steps >= 1")
    lrs = []
    for k in range(total_steps):
        if k < warmup_steps:
            lrs.append(base_lr * (k + 1) / warmup_steps)
        else:
            prog = (k + 1 - warmup_steps) / max(1, total_steps - warmup_steps)
            lrs.append(min_lr + 0.5 * (base_lr - min_lr) * (1.0 + math.cos(math.pi * prog)))
    return _built(lrs, target)


def step_decay(base_lr: float, step_size: int, gamma: float, total_steps: int, target=None):
    """``torch.optim.lr_scheduler.StepLR``: the rate is multiplied by ``gamma`` every ``step_size``
    steps (the same running product torch keeps, so the entries match it bit for bit)."""
    if total_steps < 1 or step_size < 1:
        raise ValueError("step_decay: need step_size >= 1 and total_steps >= 1")
    lrs, lr = [], float(base_lr)
    for k in range(total_steps):
        if k and k % step_size == 0:
            lr = lr * gamma
        lrs.append(lr)
    return _built(lrs, target)


def constant(base_lr: float, target=None):
    return _built([float(base_lr)], target)
