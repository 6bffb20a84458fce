"""Flat-buffer LAMB: Adam's update direction, scaled per tensor by the trust ratio of the
weights and of the update (You et al., "Large Batch Optimization for Deep Learning", 2020).

For tensor ``i`` with flat elements ``w, g, m, v`` at optimizer step ``k = t + 1``, all fp32
(``w1 = fp32(1 - beta1)``, ``b2 = fp32(beta2)``, ``w2 = fp32(1 - beta2)``):

    d   = g                       (times the clip coefficient; negated with ``maximize``)
    m'  = fma(w1, d - m, m)
    v'  = fma(w2 * d, d, b2 * v)
    den = sqrt(v') / bc2_sqrt + eps
    r   = (m' / den) * ibc1       ibc1 = fp32(1 / (1 - beta1^k)), bc2_sqrt = fp32(sqrt(1 - beta2^k))
    u   = fma(wd_i, w, r)         when wd_i != 0, else r
    phi_i = |w_i| / |u_i|         if adapt_i and both norms > 0, else 1
    w'  = fma(-(lr_t * phi_i), u, w)

* excluded tensors (``exclude="1d"``, the default: every parameter with ``ndim <= 1``;
  ``exclude=None``: none; or a callable ``(name, shape) -> bool``) have ``wd_i = 0`` and
  ``phi_i = 1``, exactly as in ``FusedLARS``;
* ``bias_correction=False`` uses ``ibc1 = bc2_sqrt = 1``;
* there is no clamp on ``|w|`` and no upper limit on ``phi``.

On the GPU two HIP kernels (csrc/kernels/lamb.hip, whose header is the definition with every
line's rounding) run the step: ``lamb_moments_kernel`` stores the new moments and leaves every
tensor's ``|w|``, ``|u|`` and ``phi`` in device memory; ``lamb_apply_kernel`` reads them there
while it updates the flat buffer and refreshes the shadow copies.  Nothing reaches the host, and
the step number, the bias corrections and the rate come from a device table indexed by the
counter the second kernel advances (:func:`lamb_coef_table`), so a captured step graph replays
each step with its own ratios and corrections.  The segment table is ``FusedLARS``'s
(:func:`~ddp_amd.ops.lars.lars_layout`).  On the CPU the same fp32 lines run as torch ops per
tensor, the norms summed in float64 and rounded once.

``FusedLAMB`` is a ``FusedAdamW``: its moments, its step counter, ``state_buffers`` /
``state_counter`` and its resume path.  ``state_dict()`` has ``torch.optim.AdamW``'s format plus
``exclude`` and ``bias_correction`` in the param group, so ``FusedAdamW`` and ``torch.optim.AdamW``
load a LAMB checkpoint and ``FusedLAMB`` loads theirs (missing keys keep the constructor's values).
"""
from __future__ import annotations

import numpy as np
import torch

from .adamw import MAX_TABLE, FusedAdamW, _f32
from .lars import SegmentTable


def lamb_coef_entry(t: int, lr_t: float, beta1: float, beta2: float, bias_correction: bool = True) -> tuple:
    """Entry ``t`` in float64: ``(ibc1, bc2_sqrt, lr, 0)`` of optimizer step ``t + 1``."""
    k = t + 1
    if not bias_correction:
        return (1.0, 1.0, lr_t, 0.0)
    return (1 / (1 - beta1 ** k), (1 - beta2 ** k) ** 0.5, lr_t, 0.0)


def _saturated(t: int, beta1: float, beta2: float, bias_correction: bool) -> bool:
    ibc1, bc2_sqrt, _, _ = lamb_coef_entry(t, 0.0, beta1, beta2, bias_correction)
    return _f32(ibc1) == 1.0 and _f32(bc2_sqrt) == 1.0


def lamb_coef_table(lr: float, betas=(0.9, 0.999), bias_correction: bool = True, lr_schedule=None,
                    max_len: int = MAX_TABLE) -> torch.Tensor:
    """The float32 ``[n, 4]`` table of :func:`lamb_coef_entry`, float64 entries rounded once.
    ``n`` is the larger of the schedule's length and ``t_sat + 1``, ``t_sat`` being the first ``t``
    at which both corrections round to 1 in float32 (0 without bias correction): every later
    entry would repeat the last one.  ``ValueError`` if that takes more than ``max_len`` entries."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    n_sched = len(lr_schedule) if lr_schedule is not None else 0
    if n_sched > max_len:
        raise ValueError(f"the lr schedule has {n_sched} steps; the LAMB coefficient table holds at most {max_len}")
    if not _saturated(max_len - 1, beta1, beta2, bias_correction):
        raise ValueError(f"betas {betas!r}: the bias corrections do not round to 1 in float32 within "
                         f"{max_len} steps, the most the LAMB coefficient table holds")
    rows = []
    t = 0
    while True:
        lr_t = lr_schedule.lr_at(t) if lr_schedule is not None else float(lr)
        rows.append(lamb_coef_entry(t, lr_t, beta1, beta2, bias_correction))
        if t >= n_sched - 1 and _saturated(t, beta1, beta2, bias_correction):
            break
        t += 1
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


class FusedLAMB(SegmentTable, FusedAdamW):
    """``FusedAdamW``'s moments, counter and state-dict format; its own update rule (per-tensor
    decay inside the update and the trust ratio), table and kernels; ``FusedLARS``'s segment table
    and trust statistics (``SegmentTable``)."""

    _norm_key = "u_norm"

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.01, exclude="1d", bias_correction: bool = True, maximize: bool = False,
                 max_grad_norm: float | None = None, lr_schedule=None):
        self.check_exclude(exclude)
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize,
                         max_grad_norm=max_grad_norm, lr_schedule=lr_schedule)
        self.param_groups[0].update(exclude=exclude, bias_correction=bool(bias_correction))
        self._init_segments()

    # ------------------------------------------------------------------ table
    def coef_table(self) -> torch.Tensor:
        if self._host_table is None:
            g = self.param_groups[0]
            self._host_table = lamb_coef_table(g["lr"], g["betas"], g["bias_correction"], self.lr_schedule)
        return self._host_table

    def hyper_changed(self):
        """The table as ``FusedAdamW``; weight_decay / exclude rewrite the per-tensor coefficients
        in place - the layout depends on the shapes alone (never inside a capture)."""
        super().hyper_changed()
        self._rewrite_segments()

    # ------------------------------------------------------------------ the step
    def _step_native(self, C):
        g = self.param_groups[0]
        fs = self.flat
        shadows = self._all_shadows()
        plan, partials, ticket, sums, trust = self._workspace(C)
        gscale = self._gscale(C)  # (grad_sqnorm first: pass 1 reads its coefficient)
        sched = self._sched_workspace()
        C.lamb_moments(fs.params, fs.grads, self.exp_avg, self.exp_avg_sq, g["betas"][0], g["betas"][1], g["eps"],
                       g["maximize"], plan, partials, ticket, sums, trust, gscale, sched)
        C.lamb(fs.params, self.exp_avg, self.exp_avg_sq, g["eps"], True, shadows, plan, trust, sched)

    def _step_torch(self):
        """The kernels' lines (lamb.hip) as fp32 torch ops: the moments over the flat buffer, then
        per tensor the update, its norm (summed in float64, rounded once) and the ratio."""
        g = self.param_groups[0]
        fs = self.flat
        p, d = fs.params, fs.grads
        if self.max_grad_norm is not None:
            d = self._clip_torch(d)
        if g["maximize"]:
            d = -d
        tab = self.coef_table()
        ibc1, bc2_sqrt, lr, _ = tab[min(self._sched_t, tab.shape[0] - 1)].tolist()
        w1, b2, w2 = _f32(1 - g["betas"][0]), _f32(g["betas"][1]), _f32(1 - g["betas"][1])
        m, v = self.exp_avg, self.exp_avg_sq
        m.add_(d - m, alpha=w1)
        v.mul_(b2).addcmul_(d, d, value=w2)
        r = (m / v.sqrt().div_(bc2_sqrt).add_(_f32(g["eps"]))).mul_(ibc1)
        wds, adapts = self._seg_coefs()
        stats = np.zeros((len(fs.names), 4), dtype=np.float32)
        f = np.float32
        for s, n in enumerate(fs.names):
            w, u = fs.view(p, n), fs.view(r, n)
            if wds[s] != 0:
                u = u.add(w, alpha=float(f(wds[s])))
            wn = f(np.sqrt(np.float64(f(w.double().square().sum().item()))))
            un = f(np.sqrt(np.float64(f(u.double().square().sum().item()))))
            phi = f(wn / un) if (adapts[s] and wn > 0 and un > 0) else f(1.0)
            stats[s] = (phi, wds[s], wn, un)
            w.add_(u, alpha=-float(f(f(lr) * phi)))
        self._host_stats = stats
        self._sched_t += 1

    # ------------------------------------------------------------------ state
    def _group_to_save(self, d: dict) -> dict:
        if callable(d["exclude"]):
            d["exclude"] = "callable"  # (a function does not belong in a checkpoint: the constructor's is kept)
        return super()._group_to_save(d)
