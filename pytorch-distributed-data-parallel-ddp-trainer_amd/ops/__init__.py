"""Ops library: HIP-kernel autograd Functions (GPU) with fp32 PyTorch references (CPU/tests)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import reference
from .adamw import FusedAdamW
from .ema import WeightEMA
from .lars import FusedLARS
from .lr_schedule import LRSchedule
from .sgd import FusedSGD


class CrossEntropyLoss(nn.Module):
    """``nn.CrossEntropyLoss(label_smoothing=eps)`` (mean) - fused HIP softmax-xent on the GPU.

    Reference: train_ddp.py:40 ``loss_fn = nn.CrossEntropyLoss()``.  ``label_smoothing`` is
    torch's: the target is ``(1 - eps) * onehot + eps / C`` over all C classes, computed inside
    the kernels' SMOOTH builds (0, the default, runs the kernels without it).  The target is an
    int64 ``[B]`` tensor or a ``data.mix.PairTarget`` (mixup / cutmix): row b then trains against
    ``w[b, 0] t(y_a[b]) + w[b, 1] t(y_b[b])``, ``t`` the smoothed one-hot - the kernels' PAIR
    builds on the GPU, ``F.cross_entropy`` with the probability target on the CPU.
    """

    def __init__(self, label_smoothing: float = 0.0):
        super().__init__()
        if not 0.0 <= label_smoothing <= 1.0:  # NaN fails too
            raise ValueError(f"label_smoothing must lie in [0, 1], got {label_smoothing!r}")
        self.label_smoothing = float(label_smoothing)

    def forward(self, logits: torch.Tensor, labels) -> torch.Tensor:
        if logits.is_cuda:
            from .functional import cross_entropy

            return cross_entropy(logits, labels, self.label_smoothing)
        if isinstance(labels, tuple):  # a PairTarget
            labels = labels.probs(logits.shape[1], logits.dtype)
        return F.cross_entropy(logits, labels, label_smoothing=self.label_smoothing)

    def extra_repr(self) -> str:
        return f"label_smoothing={self.label_smoothing}" if self.label_smoothing else ""


__all__ = ["CrossEntropyLoss", "FusedAdamW", "FusedLARS", "FusedSGD", "LRSchedule", "WeightEMA", "reference"]
