"""What the flat-buffer optimizers (``FusedSGD``, ``FusedAdamW``, ``FusedLARS``) share.

Each updates the model's one flat fp32 parameter buffer in one HIP kernel - a rule on the
streaming pass of csrc/kernels/flat_step.h - that also refreshes the shadow copies the MFMA
kernels read, and each keeps its per-step scalars in device memory so that a captured step
graph replays each step with its own values:

* the clip workspace - ``grad_sqnorm_kernel`` (csrc/kernels/grad_norm.hip) leaves the global
  norm of the flat gradient and the coefficient ``min(1, max_norm / (norm + 1e-6))`` in device
  memory and the update kernel multiplies every gradient element by it as it reads it;
* the schedule workspace - a float32 table and the ``SchedState`` words (step index, arrival
  ticket, the rate last used; csrc/kernels/types.h): the update kernel reads
  ``table[min(t, n - 1)]`` and advances ``t`` inside the same launch.  On the CPU the same table
  is indexed by a host counter;
* the conversion between the flat buffers and the per-parameter layouts of a reference
  (``torch.optim``) state dict, and the one rule for ``lr`` in it: with a schedule the saved
  ``lr`` is the rate the next step will use (as a torch scheduler leaves it) and a loaded one is
  a point of the schedule, kept in ``loaded_lr`` and not applied.
"""
from __future__ import annotations

import torch

from ..models.layers import FlatSpace, flat_space


class FlatOptimizer:
    """Base of the flat-buffer optimizers.  A subclass sets ``param_groups`` and implements
    ``step``, ``state_dict``, ``load_state_dict``, ``state_buffers`` and ``_sched_table``."""

    def _init_flat(self, model: torch.nn.Module, max_grad_norm, lr_schedule):
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm must be positive (None: no clipping)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._clip_ws = None      # GPU: (partials, ticket, stats), allocated by the first step
        self._clip_host = None    # CPU: the same four numbers
        self.lr_schedule = lr_schedule
        self._sched_ws = None     # GPU: (table, state int32[4] = SchedState t / ticket / lr_used), first step
        self._sched_t = 0         # CPU: the step index; GPU: the index the state block starts from
        self.loaded_lr = None     # the lr of the last loaded state dict (with a schedule: not applied)
        self.model = model
        self.flat: FlatSpace = flat_space(model)
        self._reg_names = [n for n, _ in model.named_parameters()]
        self.shadows: list[tuple] = []  # (off, n, bf16 dst, kind, a, b, c)
        self.steps = 0
        self.ema = None           # a WeightEMA updated as step()'s last act (attach_ema)

    # ------------------------------------------------------------------ API
    def attach_ema(self, ema):
        """``step()`` ends with ``ema.update()`` from now on (``None``: detach) - inside a
        GraphedStep capture, and with gradient accumulation on boundary steps only.  The EMA's
        ``applied()`` exchange then refreshes this optimizer's shadows too."""
        if ema is not None and ema.flat is not self.flat:
            raise ValueError("the EMA averages another model's parameters")
        if self.ema is not None:
            self.ema._opt = None
        self.ema = ema
        if ema is not None:
            ema._opt = self

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    def zero_grad(self, set_to_none: bool = True):
        # grads are views of the flat buffer: "none" is a memset that keeps the views - or no
        # memset at all when every gradient's producer overwrites it (direct_grad lazy zeroing)
        self.flat.zero_grad(lazy=True)

    def _prepare_grads(self):
        """The flat gradient buffer holds every parameter's gradient (start of ``step``)."""
        fs = self.flat
        fs.reattach_grads()
        from . import direct_grad

        direct_grad.flush_fresh(p for p, _ in fs._pairs)

    def _all_shadows(self) -> list:
        """The registered shadows plus the model's bf16 weight copy and PAD4 copies, all
        refreshed in the update pass."""
        fs = self.flat
        shadows = self.shadows
        if fs._bf16 is not None:
            shadows = shadows + [(0, fs.numel, fs._bf16, 1, 0, 0, 0)] + fs.pad4_shadows()
        return shadows

    # ------------------------------------------------------------------ clipping
    def _clip_workspace(self, C):
        """Partials, the (zeroed) arrival ticket and the ClipStats words; allocated once, by
        the first step - GraphedStep's warm-up, so before a capture."""
        if self._clip_ws is None:
            dev = self.flat.params.device
            self._clip_ws = (torch.zeros(C.GRAD_NORM_MAX_BLOCKS, dtype=torch.float32, device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev),
                             torch.zeros(4, dtype=torch.float32, device=dev))
        return self._clip_ws

    def _gscale(self, C):
        """Launch the norm kernel and return the device word holding the clip coefficient
        (``None`` without ``max_grad_norm``)."""
        if self.max_grad_norm is None:
            return None
        # the norm runs over the whole buffer: the alignment padding between
        # parameters is zero and no producer writes it
        partials, ticket, stats = self._clip_workspace(C)
        C.grad_sqnorm(self.flat.grads, self.max_grad_norm, partials, ticket, stats)
        return stats[1:2]  # ClipStats::coef, read by the kernel at run time

    def grad_clip_stats(self) -> dict | None:
        """``{"total_norm", "coef", "steps", "clipped"}`` of the clipped steps so far (the norm
        and coefficient are the last step's); one device-to-host read.  ``None`` without
        ``max_grad_norm`` or before the first step."""
        if self._clip_host is not None:
            return dict(self._clip_host)
        if self._clip_ws is None:
            return None
        s = self._clip_ws[2].cpu()
        i = s.view(torch.int32)
        return {"total_norm": s[0].item(), "coef": s[1].item(), "steps": int(i[2]), "clipped": int(i[3])}

    def _clip_torch(self, d: torch.Tensor) -> torch.Tensor:
        """The kernel's rule with torch ops: fp32 norm of the whole flat gradient (summed in
        float64, rounded once), coef = min(1, max_norm / (norm + 1e-6)) in fp32, d * coef."""
        norm = d.double().square().sum().sqrt().float()
        coef = (torch.tensor(self.max_grad_norm, dtype=torch.float32) / (norm + 1e-6)).clamp(max=1.0)
        h = self._clip_host or {"steps": 0, "clipped": 0}
        self._clip_host = {"total_norm": norm.item(), "coef": coef.item(), "steps": h["steps"] + 1,
                           "clipped": h["clipped"] + int(coef.item() < 1.0)}
        return d * coef

    # ------------------------------------------------------------------ schedule / step counter
    def _sched_table(self) -> torch.Tensor:
        """The float32 table the kernel indexes with the device counter (host tensor)."""
        return self.lr_schedule.table

    def _sched_workspace(self):
        """The float32 table and the SchedState words on the device; allocated once, by the
        first step - GraphedStep's warm-up, so before a capture (as ``_clip_workspace``)."""
        if self._sched_ws is None:
            dev = self.flat.params.device
            self._sched_ws = (self._sched_table().to(dev),
                              torch.tensor([self._sched_t, 0, 0, 0], dtype=torch.int32).to(dev))
        return self._sched_ws

    def _need_schedule(self):
        if self.lr_schedule is None:
            raise RuntimeError(f"this {type(self).__name__} has no lr_schedule")

    def schedule_step(self) -> int:
        """Optimizer steps the schedule has seen = the index of the next step's rate; on the
        GPU one device-to-host read of the counter the kernel advances."""
        self._need_schedule()
        if self._sched_ws is not None:
            return int(self._sched_ws[1][0].item())
        return self._sched_t

    def current_lr(self) -> float:
        """The rate the next step will use (the constant ``lr`` without a schedule)."""
        if self.lr_schedule is None:
            return self.param_groups[0]["lr"]
        return self.lr_schedule.lr_at(self.schedule_step())

    def set_schedule_step(self, k: int):
        """Continue the schedule at step ``k`` (resume).  On the GPU a host-to-device write of
        the counter: never inside a graph capture."""
        self._need_schedule()
        k = int(k)
        if k < 0:
            raise ValueError("the schedule step must be >= 0")
        self._sched_t = k
        if self._sched_ws is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("set_schedule_step inside a graph capture")
            self._sched_ws[1].copy_(torch.tensor([k, 0, 0, 0], dtype=torch.int32))

    # ------------------------------------------------------------------ state dict
    def _group_to_save(self, d: dict) -> dict:
        """``d`` - the group's hyper-parameters under the reference's keys, in its order - as the
        param group of a state dict."""
        if self.lr_schedule is not None:
            d["lr"] = self.current_lr()
        d["params"] = list(range(len(self._reg_names)))
        return d

    def _saved_group(self, sd) -> dict:
        """The one param group of a state dict for this model."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._reg_names):
            raise ValueError("optimizer state_dict does not match this model")
        return groups[0]

    def _load_group(self, saved: dict, keys):
        """Take the hyper-parameters ``keys`` that ``saved`` has (missing ones keep their values)."""
        g = self.param_groups[0]
        for k in keys:
            if k == "lr" and self.lr_schedule is not None:
                # a checkpoint's lr is a point of the schedule: the base is the constructor's
                self.loaded_lr = saved.get("lr")  # (kept so a resume can check its step index)
            elif k in saved:
                g[k] = saved[k]


def _owner(model, name):
    mod = model
    for p in name.split(".")[:-1]:
        mod = getattr(mod, p)
    return mod, name.split(".")[-1]


def _to_reference_layout(model, fs: FlatSpace, flat_buf: torch.Tensor) -> dict:
    """Per-parameter tensors of ``flat_buf`` in the layout the reference state_dict uses."""
    from ..models.layers import Conv2d, Linear

    out = {}
    for n in fs.names:
        v = fs.view(flat_buf, n).detach()
        mod, attr = _owner(model, n)
        if attr == "weight" and isinstance(mod, Conv2d):
            v = v.permute(0, 3, 1, 2)
        elif attr == "weight" and isinstance(mod, Linear) and mod.in_layout is not None:
            C, H, W = mod.in_layout
            v = v.permute(0, 2, 1).reshape(mod.out_features, C * H * W)
        out[n] = v.contiguous().clone()
    return out


def _from_reference_layout(model, fs: FlatSpace, ref: dict, flat_buf: torch.Tensor):
    from ..models.layers import Conv2d, Linear

    for n, v in ref.items():
        mod, attr = _owner(model, n)
        if attr == "weight" and isinstance(mod, Conv2d):
            v = v.permute(0, 2, 3, 1)
        elif attr == "weight" and isinstance(mod, Linear) and mod.in_layout is not None:
            C, H, W = mod.in_layout
            v = v.reshape(mod.out_features, C, H * W).permute(0, 2, 1)
        fs.view(flat_buf, n).copy_(v)
