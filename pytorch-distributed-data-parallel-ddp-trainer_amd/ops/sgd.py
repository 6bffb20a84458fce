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

from .flat_optim import FlatOptimizer, _from_reference_layout, _to_reference_layout

_DEFAULTS = dict(lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False,
                 maximize=False, foreach=None, differentiable=False, fused=None)


class FusedSGD(FlatOptimizer):
    """Also the base of ``FusedLARS`` (ops/lars.py), which keeps the momentum state, its state
    dict and the momentum half of the CPU step, and replaces the gradient rule and the launch."""

    _group_keys = tuple(_DEFAULTS)  # the param group's keys in a state dict, in order

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, momentum: float = 0,
                 dampening: float = 0, weight_decay: float = 0, nesterov: bool = False,
                 maximize: bool = False, max_grad_norm: float | None = None, lr_schedule=None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._init_flat(model, max_grad_norm, lr_schedule)
        g = dict(_DEFAULTS)
        g.update(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                 nesterov=nesterov, maximize=maximize)
        self.param_groups = [g]
        self.momentum_buffer: torch.Tensor | None = None

    # ------------------------------------------------------------------ API
    @torch.no_grad()
    def step(self):
        fs = self.flat
        self._prepare_grads()
        first = self.momentum_buffer is None
        if self.param_groups[0]["momentum"] != 0 and first:
            self.momentum_buffer = torch.zeros_like(fs.params)
        if fs.params.is_cuda:
            from .. import native

            self._step_native(native.require(), first)
            fs.mark_bf16_fresh()
        else:
            self._step_torch(first)
        self.steps += 1
        if self.ema is not None:
            self.ema.update()

    def _step_native(self, C, first: bool):
        g = self.param_groups[0]
        fs = self.flat
        shadows = self._all_shadows()  # incl. the model's bf16 weight copy, refreshed in the same pass
        gscale = self._gscale(C)
        # with a schedule every step, eager or captured, runs the DLR build: one device counter
        sched = self._sched_workspace() if self.lr_schedule is not None else None
        C.sgd(fs.params, fs.grads, self.momentum_buffer, g["lr"], g["momentum"],
              g["dampening"], g["weight_decay"], g["nesterov"], g["maximize"],
              first, True, shadows, gscale, sched)

    def state_buffers(self) -> dict:
        """The optimizer state as named flat tensors (``None``: not created yet) - what a
        resume broadcasts and ``--verify_replicas`` hashes."""
        return {"momentum_buffer": self.momentum_buffer}

    def set_state_buffer(self, name: str, buf: torch.Tensor):
        assert name == "momentum_buffer"
        self.momentum_buffer = buf

    def _grad_torch(self) -> torch.Tensor:
        """The (clipped, with ``maximize`` negated) gradient plus the weight decay, a new tensor."""
        g = self.param_groups[0]
        p, d = self.flat.params, self.flat.grads
        if self.max_grad_norm is not None:
            d = self._clip_torch(d)
        d = -d if g["maximize"] else d.clone()
        if g["weight_decay"] != 0:
            d = d.add(p, alpha=g["weight_decay"])
        return d

    def _step_torch(self, first: bool):
        g = self.param_groups[0]
        d = self._grad_torch()
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
        self.flat.params.add_(d, alpha=-lr)

    # ------------------------------------------------------------------ state
    def _group_values(self) -> dict:
        g = self.param_groups[0]
        return {k: g[k] for k in self._group_keys}

    def state_dict(self):
        state = {}
        if self.momentum_buffer is not None:
            ref = _to_reference_layout(self.model, self.flat, self.momentum_buffer)
            for i, n in enumerate(self._reg_names):
                state[i] = {"momentum_buffer": ref[n]}
        return {"state": state, "param_groups": [self._group_to_save(self._group_values())]}

    def load_state_dict(self, sd):
        self._load_group(self._saved_group(sd), self._group_keys)
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
