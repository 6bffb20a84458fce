"""Flat-buffer SGD with ``torch.optim.SGD`` semantics and state_dict format.

Reference: ``optim.SGD(model.parameters(), lr=0.01)`` (train_ddp.py:41) and
``opt.step()`` (train_ddp.py:200).  On the GPU one HIP kernel (``sgd_kernel`` in
csrc/kernels/optim.hip) updates the whole flat parameter buffer of the model
(weight decay / momentum / dampening / nesterov / maximize as in
torch/optim/sgd.py ``_single_tensor_sgd``) and refreshes any registered bf16
shadow copies in the same pass.  On the CPU the identical math runs as torch ops
over the same flat buffers.

``state_dict()`` reproduces ``torch.optim.SGD.state_dict()`` exactly (same
``param_groups`` keys and order, ``params`` = registration-order indices, and
``momentum_buffer`` tensors in the reference layout), so checkpoints stay
byte-compatible with the reference.

``max_grad_norm`` adds ``torch.nn.utils.clip_grad_norm_`` (norm_type 2) to the step itself:
``grad_sqnorm_kernel`` (csrc/kernels/grad_norm.hip) leaves the global norm of the flat
gradient and the coefficient ``min(1, max_norm / (norm + 1e-6))`` in device memory, and the
CLIP build of ``sgd_kernel`` multiplies every gradient element by it as it reads it.  The
gradient buffer is not rewritten and nothing reaches the host, so a captured graph replays
the step with each batch's own coefficient.  Clipping is configured by the constructor only
and keeps no optimizer state (torch keeps none either): ``state_dict()`` is unchanged.

``lr_schedule`` (an :class:`~ddp_amd.ops.lr_schedule.LRSchedule`) makes the rate a function of
the optimizer-step index.  On the GPU the float32 table and a small state block (step index,
arrival ticket, the rate last used) live in device memory: the DLR build of ``sgd_kernel``
reads ``table[min(t, n - 1)]`` at run time and advances ``t`` inside the same launch, so eager
steps and replays of a captured graph share one counter and every step gets its own rate.
On the CPU the same table is indexed by a host counter.  The schedule adds no checkpoint
field: ``state_dict()`` keeps its keys, its ``lr`` is the rate the next step will use (as a
torch scheduler leaves it), and a resumed run restores the index with ``set_schedule_step``.
"""
from __future__ import annotations

import torch

from ..models.layers import FlatSpace, flat_space

_DEFAULTS = dict(lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False,
                 maximize=False, foreach=None, differentiable=False, fused=None)


class FusedSGD:
    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, momentum: float = 0,
                 dampening: float = 0, weight_decay: float = 0, nesterov: bool = False,
                 maximize: bool = False, max_grad_norm: float | None = None, lr_schedule=None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
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
        g = dict(_DEFAULTS)
        g.update(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                 nesterov=nesterov, maximize=maximize)
        self.param_groups = [g]
        self._reg_names = [n for n, _ in model.named_parameters()]
        self.momentum_buffer: torch.Tensor | None = None
        self.shadows: list[tuple] = []  # (off, n, bf16 dst, kind, a, b, c)
        self.steps = 0

    # ------------------------------------------------------------------ API
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    def zero_grad(self, set_to_none: bool = True):
        # grads are views of the flat buffer: "none" is a memset that keeps the views - or no
        # memset at all when every gradient's producer overwrites it (direct_grad lazy zeroing)
        self.flat.zero_grad(lazy=True)

    @torch.no_grad()
    def step(self):
        g = self.param_groups[0]
        fs = self.flat
        fs.reattach_grads()
        from . import direct_grad

        direct_grad.flush_fresh(p for p, _ in fs._pairs)
        first = self.momentum_buffer is None
        if g["momentum"] != 0 and first:
            self.momentum_buffer = torch.zeros_like(fs.params)
        if fs.params.is_cuda:
            from .. import native

            shadows = self.shadows
            if fs._bf16 is not None:  # the model's bf16 weight copy, refreshed in the same pass
                shadows = shadows + [(0, fs.numel, fs._bf16, 1, 0, 0, 0)] + fs.pad4_shadows()
            C = native.require()
            gscale = None
            if self.max_grad_norm is not None:
                # the norm runs over the whole buffer: the alignment padding between
                # parameters is zero and no producer writes it
                partials, ticket, stats = self._clip_workspace(C)
                C.grad_sqnorm(fs.grads, self.max_grad_norm, partials, ticket, stats)
                gscale = stats[1:2]  # ClipStats::coef, read by the kernel at run time
            # with a schedule every step, eager or captured, runs the DLR build: one device counter
            sched = self._sched_workspace() if self.lr_schedule is not None else None
            C.sgd(fs.params, fs.grads, self.momentum_buffer, g["lr"], g["momentum"],
                  g["dampening"], g["weight_decay"], g["nesterov"], g["maximize"],
                  first, True, shadows, gscale, sched)
            fs.mark_bf16_fresh()
        else:
            self._step_torch(first)
        self.steps += 1

    def _clip_workspace(self, C):
        """Partials, the (zeroed) arrival ticket and the ClipStats words; allocated once, by
        the first step - GraphedStep's warm-up, so before a capture."""
        if self._clip_ws is None:
            dev = self.flat.params.device
            self._clip_ws = (torch.zeros(C.GRAD_NORM_MAX_BLOCKS, dtype=torch.float32, device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev),
                             torch.zeros(4, dtype=torch.float32, device=dev))
        return self._clip_ws

    def _sched_workspace(self):
        """The float32 table and the SchedState words on the device; allocated once, by the
        first step - GraphedStep's warm-up, so before a capture (as ``_clip_workspace``)."""
        if self._sched_ws is None:
            dev = self.flat.params.device
            self._sched_ws = (self.lr_schedule.table.to(dev),
                              torch.tensor([self._sched_t, 0, 0, 0], dtype=torch.int32).to(dev))
        return self._sched_ws

    def _need_schedule(self):
        if self.lr_schedule is None:
            raise RuntimeError("this FusedSGD has no lr_schedule")

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

    def _step_torch(self, first: bool):
        g = self.param_groups[0]
        p, d = self.flat.params, self.flat.grads
        if self.max_grad_norm is not None:
            d = self._clip_torch(d)
        d = -d if g["maximize"] else d.clone()
        if g["weight_decay"] != 0:
            d = d.add(p, alpha=g["weight_decay"])
        if g["momentum"] != 0:
            buf = self.momentum_buffer
            if first:
                buf.copy_(d)
            else:
                buf.mul_(g["momentum"]).add_(d, alpha=1 - g["dampening"])
            d = d.add(buf, alpha=g["momentum"]) if g["nesterov"] else buf
        lr = g["lr"]
        if self.lr_schedule is not None:
            lr = self.lr_schedule.lr_at(self._sched_t)
            self._sched_t += 1
        p.add_(d, alpha=-lr)

    # ------------------------------------------------------------------ state
    def state_dict(self):
        state = {}
        if self.momentum_buffer is not None:
            ref = _to_reference_layout(self.model, self.flat, self.momentum_buffer)
            for i, n in enumerate(self._reg_names):
                state[i] = {"momentum_buffer": ref[n]}
        groups = []
        for g in self.param_groups:
            d = {k: g[k] for k in _DEFAULTS}
            if self.lr_schedule is not None:
                d["lr"] = self.current_lr()
            d["params"] = list(range(len(self._reg_names)))
            groups.append(d)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._reg_names):
            raise ValueError("optimizer state_dict does not match this model")
        for k in _DEFAULTS:
            if k == "lr" and self.lr_schedule is not None:
                # a checkpoint's lr is a point of the schedule: the base is the constructor's
                self.loaded_lr = groups[0].get("lr")  # (kept so a resume can check its step index)
                continue
            if k in groups[0]:
                self.param_groups[0][k] = groups[0][k]
        st = sd.get("state", {})
        if st:
            buf = torch.zeros_like(self.flat.params)
            ref = {self._reg_names[int(i)]: v["momentum_buffer"] for i, v in st.items()
                   if "momentum_buffer" in v}
            _from_reference_layout(self.model, self.flat, ref, buf)
            self.momentum_buffer = buf
            # torch only creates a momentum buffer in its first step: a loaded buffer means
            # the next step is a regular update (buf = m*buf + (1-d)*g), never the
            # initialisation step (buf = g) - the fused engine keys that off ``steps``
            self.steps = max(self.steps, 1)
        else:
            self.momentum_buffer = None
            self.steps = 0

    def mark_started(self):
        """A momentum buffer arrived from elsewhere (resume broadcast): treat as started."""
        if self.momentum_buffer is not None:
            self.steps = max(self.steps, 1)


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
