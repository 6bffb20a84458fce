"""Flat-buffer AdamW with ``torch.optim.AdamW`` semantics and state_dict format.

On the GPU one HIP kernel (``adamw_kernel`` in csrc/kernels/adamw.hip) updates the whole flat
parameter buffer and both moment buffers (decoupled weight decay, bias correction, maximize as
in torch/optim/adam.py ``_single_tensor_adam``; no amsgrad) and refreshes the shadow copies the
MFMA kernels read in the same pass, exactly as ``FusedSGD``'s ``sgd_kernel`` does.  On the CPU
the same operation sequence runs as torch ops over the same flat buffers.

Bias correction needs the step number, and a captured step graph replays one launch, so the
step number lives in device memory (the ``SchedState`` words ``FusedSGD`` uses for its
learning-rate schedule) and the kernel advances it itself.  Everything that depends on it comes
from a device-resident table (:func:`coef_table`): entry ``t`` holds, for optimizer step
``k = t + 1`` with rate ``lr_t``,

    decay     = 1 - lr_t * weight_decay
    step_size = lr_t / (1 - beta1 ** k)
    bc2_sqrt  = (1 - beta2 ** k) ** 0.5
    lr        = lr_t

computed in Python float64 and rounded once to float32 - the values torch's single-tensor path
forms as Python scalars and hands to its fp32 kernels.  ``lr_t`` is the ``lr_schedule``'s
float32 entry ``min(t, n - 1)``, else the constant ``lr``: the Adam step and the schedule index
are one counter.  The table ends where its entries stop changing (both corrections round to 1
in float32; never before the schedule's end); past it the last entry holds, so clamping the
index is exact.

``state_dict()`` has the format of the installed ``torch.optim.AdamW`` (its ``param_groups``
keys in its order, ``state[i] = {"step", "exp_avg", "exp_avg_sq"}`` in the reference layouts),
so either optimizer loads the other's.  The step counter is part of the state: a resumed run
continues from the checkpoint's ``step``.  ``max_grad_norm`` and ``lr_schedule`` work as in
``FusedSGD`` and add no state.
"""
from __future__ import annotations

import struct

import torch

from .flat_optim import FlatOptimizer, _from_reference_layout, _to_reference_layout

MAX_TABLE = 1 << 20


def _f32(x: float) -> float:
    """``x`` rounded once to float32 (round to nearest even), as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


def coef_entry(t: int, lr_t: float, beta1: float, beta2: float, weight_decay: float) -> tuple:
    """Entry ``t`` in float64: ``(decay, step_size, bc2_sqrt, lr)`` of optimizer step ``t + 1``."""
    k = t + 1
    return (1 - lr_t * weight_decay, lr_t / (1 - beta1 ** k), (1 - beta2 ** k) ** 0.5, lr_t)


def _saturated(t: int, lr_t: float, beta1: float, beta2: float) -> bool:
    _, step_size, bc2_sqrt, _ = coef_entry(t, lr_t, beta1, beta2, 0.0)
    return _f32(step_size) == _f32(lr_t) and _f32(bc2_sqrt) == 1.0


def coef_table(lr: float, betas=(0.9, 0.999), weight_decay: float = 1e-2, lr_schedule=None,
               max_len: int = MAX_TABLE) -> torch.Tensor:
    """The float32 ``[n, 4]`` table of :func:`coef_entry`.  ``n`` is the larger of the
    schedule's length and ``t_sat + 1``, ``t_sat`` being the first ``t`` whose float32 entry
    has both bias corrections rounded away (``step_size == lr`` and ``bc2_sqrt == 1``): every
    later entry would repeat the last one.  ``ValueError`` if that takes more than ``max_len``
    entries."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    n_sched = len(lr_schedule) if lr_schedule is not None else 0
    if n_sched > max_len:
        raise ValueError(f"the lr schedule has {n_sched} steps; the AdamW coefficient table holds at most {max_len}")

    def lr_at(t):
        return lr_schedule.lr_at(t) if lr_schedule is not None else float(lr)

    if not _saturated(max_len - 1, lr_at(max_len - 1), beta1, beta2):
        raise ValueError(f"betas {betas!r}: the bias corrections do not round to 1 in float32 within "
                         f"{max_len} steps, the most the AdamW coefficient table holds")
    rows = []
    t = 0
    while True:
        lr_t = lr_at(t)
        rows.append(coef_entry(t, lr_t, beta1, beta2, float(weight_decay)))
        if t >= n_sched - 1 and _saturated(t, lr_t, beta1, beta2):
            break
        t += 1
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


def _torch_defaults(**kw) -> dict:
    """``param_groups[0]`` of a throwaway ``torch.optim.AdamW``: the installed torch's keys, in
    its order, with its defaults (``params`` left out)."""
    g = dict(torch.optim.AdamW([torch.zeros(1)], **kw).param_groups[0])
    g.pop("params")
    return g


class FusedAdamW(FlatOptimizer):
    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, maximize: bool = False, max_grad_norm: float | None = None,
                 lr_schedule=None):
        # (torch's own checks of lr / betas / eps / weight_decay run here)
        g = _torch_defaults(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                            weight_decay=float(weight_decay), maximize=bool(maximize))
        self._init_flat(model, max_grad_norm, lr_schedule)
        self.param_groups = [g]
        self.exp_avg: torch.Tensor | None = None
        self.exp_avg_sq: torch.Tensor | None = None
        self._host_table = None  # float32 [n, 4], built by the first step (or schedule query)

    # ------------------------------------------------------------------ table / counter
    def coef_table(self) -> torch.Tensor:
        if self._host_table is None:
            g = self.param_groups[0]
            self._host_table = coef_table(g["lr"], g["betas"], g["weight_decay"], self.lr_schedule)
        return self._host_table

    def _sched_table(self):
        return self.coef_table()

    def _need_schedule(self):
        pass  # the counter is the Adam step: there with or without an lr_schedule

    def hyper_changed(self):
        """The table is a function of lr / betas / weight_decay: rebuild it, in place on the
        device when it keeps its size (never inside a capture)."""
        self._host_table = None
        if self._sched_ws is not None:
            new = self.coef_table()
            if new.shape == self._sched_ws[0].shape:
                self._sched_ws[0].copy_(new)
            else:
                self._sched_t = self.schedule_step()
                self._sched_ws = None

    # ------------------------------------------------------------------ API
    @torch.no_grad()
    def step(self):
        g = self.param_groups[0]
        fs = self.flat
        self._prepare_grads()
        if self.exp_avg is None:  # (the first step: GraphedStep's warm-up, so before a capture)
            self.exp_avg = torch.zeros_like(fs.params)
            self.exp_avg_sq = torch.zeros_like(fs.params)
        if fs.params.is_cuda:
            from .. import native

            shadows = self._all_shadows()
            C = native.require()
            gscale = self._gscale(C)
            C.adamw(fs.params, fs.grads, self.exp_avg, self.exp_avg_sq, g["betas"][0], g["betas"][1],
                    g["eps"], g["maximize"], True, shadows, gscale, self._sched_workspace())
            fs.mark_bf16_fresh()
        else:
            self._step_torch()
        self.steps += 1
        if self.ema is not None:
            self.ema.update()

    def _step_torch(self):
        """The kernel's operation sequence (adamw.hip) as fp32 torch ops, the scalars from the
        same float32 table indexed by the host counter."""
        g = self.param_groups[0]
        p, d = self.flat.params, self.flat.grads
        if self.max_grad_norm is not None:
            d = self._clip_torch(d)
        if g["maximize"]:
            d = -d
        tab = self.coef_table()
        decay, step_size, bc2_sqrt, _ = tab[min(self._sched_t, tab.shape[0] - 1)].tolist()
        w1, b2, w2 = _f32(1 - g["betas"][0]), _f32(g["betas"][1]), _f32(1 - g["betas"][1])
        m, v = self.exp_avg, self.exp_avg_sq
        p.mul_(decay)
        m.add_(d - m, alpha=w1)
        v.mul_(b2).addcmul_(d, d, value=w2)
        den = v.sqrt().div_(bc2_sqrt).add_(_f32(g["eps"]))
        p.addcdiv_(m, den, value=-step_size)
        self._sched_t += 1

    # ------------------------------------------------------------------ state
    def state_buffers(self) -> dict:
        """The optimizer state as named flat tensors (``None``: not created yet) - what a
        resume broadcasts and ``--verify_replicas`` hashes."""
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}

    def set_state_buffer(self, name: str, buf: torch.Tensor):
        assert name in ("exp_avg", "exp_avg_sq")
        setattr(self, name, buf)

    def state_counter(self) -> int:
        return self.schedule_step()

    def set_state_counter(self, k: int):
        self.set_schedule_step(k)
        self.steps = int(k)

    def state_dict(self):
        state = {}
        if self.exp_avg is not None:
            step = float(self.schedule_step())
            m = _to_reference_layout(self.model, self.flat, self.exp_avg)
            v = _to_reference_layout(self.model, self.flat, self.exp_avg_sq)
            for i, n in enumerate(self._reg_names):
                state[i] = {"step": torch.tensor(step, dtype=torch.float32), "exp_avg": m[n], "exp_avg_sq": v[n]}
        return {"state": state, "param_groups": [self._group_to_save(dict(self.param_groups[0]))]}

    def load_state_dict(self, sd):
        saved = self._saved_group(sd)
        if saved.get("amsgrad"):
            raise ValueError("FusedAdamW does not support amsgrad=True")
        g = self.param_groups[0]
        self._load_group(saved, list(g))
        g["betas"] = tuple(g["betas"])
        self.hyper_changed()
        st = sd.get("state", {})
        if st:
            m, v = torch.zeros_like(self.flat.params), torch.zeros_like(self.flat.params)
            names = {int(i): self._reg_names[int(i)] for i in st}
            _from_reference_layout(self.model, self.flat, {names[int(i)]: s["exp_avg"] for i, s in st.items()}, m)
            _from_reference_layout(self.model, self.flat, {names[int(i)]: s["exp_avg_sq"] for i, s in st.items()}, v)
            self.exp_avg, self.exp_avg_sq = m, v
            self.set_state_counter(int(float(st[min(st, key=int)]["step"])))
        else:
            self.exp_avg = self.exp_avg_sq = None
            self.set_state_counter(0)
