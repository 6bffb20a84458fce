"""Learning-rate schedules as a table: one value per optimizer step.

``LRSchedule`` evaluates a closed form (linear warm-up, then cosine, linear or step decay)
once on the host, in float64, for every optimizer step ``t = 0 .. total_steps - 1``:

    t < warmup_steps   base * (warmup_start + (1 - warmup_start) * t / warmup_steps)
    otherwise, with k = t - warmup_steps and T = max(1, total_steps - warmup_steps)
      cosine           lr_min + (base - lr_min) * (1 + cos(pi k / T)) / 2
      linear           base + (lr_min - base) * k / T
      step             base * gamma ** (k // step_size)
      none             base

(``torch.optim.lr_scheduler`` CosineAnnealingLR / LinearLR / StepLR behind a SequentialLR
LinearLR warm-up, in closed form.)  ``table`` is the float32 rounding of those values - the
single rounding a by-value ``lr`` gets on its way into ``sgd_kernel`` - and is what
``FusedSGD(lr_schedule=...)`` uploads: the DLR build of ``sgd_kernel`` indexes it with a
device-resident step counter, so a captured step graph follows the schedule.  Past the end
of the table the last entry holds.

The schedule is a pure function of its arguments and the global optimizer-step index: every
rank builds the same table from the same flags, and a resumed run only needs the index.
"""
from __future__ import annotations

import math

import torch

KINDS = ("none", "cosine", "linear", "step")


class LRSchedule:
    def __init__(self, base_lr: float, total_steps: int, kind: str = "none", warmup_steps: int = 0,
                 warmup_start: float = 0.01, lr_min: float = 0.0, step_size: int = 0, gamma: float = 0.1):
        if kind not in KINDS:
            raise ValueError(f"unknown lr schedule {kind!r} (one of {', '.join(KINDS)})")
        total_steps, warmup_steps, step_size = int(total_steps), int(warmup_steps), int(step_size)
        if total_steps < 1:
            raise ValueError("an lr schedule needs total_steps >= 1")
        if warmup_steps < 0:
            raise ValueError("warmup_steps must be >= 0")
        if kind == "step" and step_size < 1:
            raise ValueError("the step schedule needs step_size >= 1")
        base, lr_min = float(base_lr), float(lr_min)
        T = max(1, total_steps - warmup_steps)
        vals = []
        for t in range(total_steps):
            if t < warmup_steps:
                v = base * (warmup_start + (1 - warmup_start) * t / warmup_steps)
            else:
                k = t - warmup_steps
                if kind == "cosine":
                    v = lr_min + (base - lr_min) * (1 + math.cos(math.pi * k / T)) / 2
                elif kind == "linear":
                    v = base + (lr_min - base) * k / T
                elif kind == "step":
                    v = base * gamma ** (k // step_size)
                else:
                    v = base
            vals.append(v)
        self.kind, self.base_lr, self.total_steps, self.warmup_steps = kind, base, total_steps, warmup_steps
        self._set(vals)

    @classmethod
    def from_values(cls, seq) -> "LRSchedule":
        """A schedule from precomputed per-step rates (e.g. recorded from a
        ``torch.optim.lr_scheduler``)."""
        vals = [float(v) for v in seq]
        if not vals:
            raise ValueError("an lr schedule needs at least one value")
        self = cls.__new__(cls)
        self.kind, self.base_lr, self.total_steps, self.warmup_steps = "values", vals[0], len(vals), 0
        self._set(vals)
        return self

    def _set(self, vals):
        self.values = torch.tensor(vals, dtype=torch.float64)   # the closed form, float64
        if not bool(torch.isfinite(self.values).all()):
            raise ValueError("lr schedule values must be finite")
        self.table = self.values.to(torch.float32)              # what the optimizer uses

    def __len__(self) -> int:
        return self.total_steps

    def lr_at(self, t: int) -> float:
        """The rate of optimizer step ``t`` (a float32 value; the last entry past the end)."""
        return float(self.table[min(max(int(t), 0), self.total_steps - 1)])
