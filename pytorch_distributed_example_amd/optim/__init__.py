"""Fused optimizers (one HIP launch per step over a flat buffer), torch.optim-compatible state, and
``lr_scheduler``: per-step learning-rate tables the kernels read on the device (schedules under hipGraph)."""
from .fused import SGD, Adam, AdamW  # noqa: F401
from .master import AdamWMaster, SGDMaster  # noqa: F401
from . import lr_scheduler  # noqa: F401
from .lr_scheduler import LRTable  # noqa: F401
