"""Flat-buffer LARS: SGD with momentum whose per-tensor decayed gradient is scaled by a trust ratio.

For tensor ``i`` of the model, with flat elements ``w`` and ``g``:

* excluded tensors (``exclude="1d"``: every parameter with ``ndim <= 1`` - BatchNorm scales and
  biases, every bias; ``exclude=None``: none; or a callable ``(name, shape) -> bool``) have
  ``wd_i = 0`` and ``ratio_i = 1``: plain SGD without decay;
* adapted tensors have ``wd_i = weight_decay`` and, with ``wn = sqrt(sum w^2)`` and
  ``gn = sqrt(sum g^2)`` (each root correctly rounded in fp32; with clipping ``gn`` is then
  multiplied once by the clip coefficient - the norm of the gradient the update sees),

      ratio_i = (trust_coef * wn) / (fma(wd_i, wn, gn) + eps)   if wn > 0 and gn > 0, else 1

* per element, in this order: ``d = g`` (times the clip coefficient; negated with
  ``maximize``), ``d = fma(wd_i, w, d)`` when ``wd_i != 0``, ``d = d * ratio_i``, then the
  momentum / dampening / nesterov lines of SGD, then ``w = fma(-lr_t, d, w)``.  With
  ``ratio_i = 1`` this is ``FusedSGD``'s update bit for bit.

On the GPU two HIP kernels (csrc/kernels/lars.hip) run the step: ``seg_sqnorm_kernel`` leaves
every tensor's norms and ratio in device memory and ``lars_kernel`` reads them there while it
updates the flat buffer and refreshes the shadow copies, so nothing reaches the host and a
captured step graph replays each step with its own ratios.  They find a quad's tensor through
a segment table (:func:`lars_layout`) built once from the parameter shapes.  On the CPU the
same rule runs with torch ops per tensor, the norms summed in float64 and rounded once.

``state_dict()`` has ``torch.optim.SGD``'s format (``momentum_buffer`` per parameter in the
reference layouts; the one param group has SGD's keys in SGD's order, then ``trust_coef``,
``eps``, ``exclude``), so ``FusedSGD`` and ``torch.optim.SGD`` load a LARS checkpoint and
``FusedLARS`` loads theirs (missing keys keep the constructor's values).  ``max_grad_norm`` and
``lr_schedule`` work as in ``FusedSGD`` and add no state.
"""
from __future__ import annotations

import numpy as np
import torch

from . import kernel_bounds as kb
from .sgd import _DEFAULTS, FusedSGD

ITEM, CHUNK, MAX_SEGS = kb.LARS_ITEM, kb.LARS_CHUNK, kb.LARS_MAX_SEGS  # csrc/kernels/launchers.h
_EXTRA = ("trust_coef", "eps", "exclude")


def lars_layout(begins, numels, n: int, wds, adapts):
    """The segment table of lars.hip for tensors at flat offsets ``begins`` (ascending, each a
    multiple of 64) with ``numels`` elements in a buffer of ``n``: ``(segs int32 [n_seg, 8],
    items int32 [n_items, 4], cmap int16 [ceil(n / 64)])`` as host tensors.  A function of the
    arguments alone."""
    n_seg = len(begins)
    if not 1 <= n_seg <= MAX_SEGS:
        raise ValueError(f"LARS handles 1 .. {MAX_SEGS} parameter tensors, got {n_seg}")
    segs = np.zeros((n_seg, 8), dtype=np.int32)
    items = []
    cmap = np.full(-(-n // CHUNK), n_seg, dtype=np.int16)
    end = 0
    for s, (b, m) in enumerate(zip(begins, numels)):
        if b % CHUNK or b < end or b + m > n:
            raise ValueError("LARS needs every tensor on its own 64-element boundary of the flat buffer")
        end = b + m
        k_n = -(-m // ITEM)
        segs[s, :4] = (b // CHUNK, m, len(items), k_n)
        segs[s, 4] = np.float32(wds[s]).view(np.int32)
        segs[s, 5] = int(bool(adapts[s]))
        items += [(b // CHUNK + k * (ITEM // CHUNK), min(ITEM, m - k * ITEM), s, k) for k in range(k_n)]
        cmap[b // CHUNK:-(-(b + m) // CHUNK)] = s
    items = np.asarray(items, dtype=np.int32).reshape(-1, 4)
    return torch.from_numpy(segs), torch.from_numpy(items), torch.from_numpy(cmap)


class FusedLARS(FusedSGD):
    """``FusedSGD``'s momentum state, state-dict format and momentum step; its own gradient rule
    (per-tensor decay and trust ratio) and kernels."""

    _group_keys = (*_DEFAULTS, *_EXTRA)

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, momentum: float = 0.9, dampening: float = 0,
                 weight_decay: float = 0, nesterov: bool = False, maximize: bool = False,
                 trust_coef: float = 1e-3, eps: float = 1e-8, exclude="1d",
                 max_grad_norm: float | None = None, lr_schedule=None):
        if not trust_coef > 0:
            raise ValueError("trust_coef must be positive")
        if eps < 0 or weight_decay < 0:
            raise ValueError("eps and weight_decay must be >= 0")
        if not (exclude is None or exclude == "1d" or callable(exclude)):
            raise ValueError("exclude must be '1d', None or a callable (name, shape) -> bool")
        super().__init__(model, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov, maximize=maximize, max_grad_norm=max_grad_norm, lr_schedule=lr_schedule)
        self.param_groups[0].update(trust_coef=trust_coef, eps=eps, exclude=exclude)
        self._excluded_wd = 0.0   # decay of the excluded tensors (0 by definition; the SGD-anchor test forces it)
        self._ws = None           # GPU: (plan, partials, ticket, sums, trust), allocated by the first step
        self._host_stats = None   # CPU: float32 [n_seg, 4] {ratio, wd, wn, gn} of the last step

    # ------------------------------------------------------------------ segments
    def excluded(self, name: str) -> bool:
        ex = self.param_groups[0]["exclude"]
        shape = self.flat.shapes[name]
        if ex is None:
            return False
        if callable(ex):
            return bool(ex(name, shape))
        return len(shape) <= 1

    def _seg_coefs(self):
        """Per tensor, in flat order: (wd_i, adapt_i)."""
        wd = float(self.param_groups[0]["weight_decay"])
        ex = [self.excluded(n) for n in self.flat.names]
        return [self._excluded_wd if e else wd for e in ex], [not e for e in ex]

    def layout(self):
        fs = self.flat
        wds, adapts = self._seg_coefs()
        return lars_layout([fs.offsets[n] for n in fs.names], [fs.numels[n] for n in fs.names], fs.numel, wds, adapts)

    def _workspace(self, C):
        """The plan (segment table on the device), the item partials, the (zeroed) arrival
        ticket, the per-tensor sums and the trust table; allocated once, by the first step -
        GraphedStep's warm-up, so before a capture."""
        if self._ws is None:
            fs = self.flat
            dev = fs.params.device
            segs, items, cmap = self.layout()
            plan = C.lars_plan(segs, items, cmap, fs.numel, fs.params)
            n_seg = segs.shape[0]
            trust = torch.zeros(n_seg + 1, 4, dtype=torch.float32)
            trust[n_seg, 0] = 1.0  # the null segment (padding): ratio 1, wd 0
            self._ws = (plan, torch.zeros(2 * max(items.shape[0], 1), dtype=torch.float32, device=dev),
                        torch.zeros(1, dtype=torch.int32, device=dev),
                        torch.zeros(n_seg, 2, dtype=torch.float32, device=dev), trust.to(dev))
        return self._ws

    def hyper_changed(self):
        """weight_decay / exclude changed (a loaded state dict): rewrite the per-tensor
        coefficients in place - the layout depends on the shapes alone (never inside a capture)."""
        if self._ws is not None:
            self._ws[0][0].copy_(self.layout()[0])

    # ------------------------------------------------------------------ the step
    def _step_native(self, C, first: bool):
        g = self.param_groups[0]
        fs = self.flat
        shadows = self._all_shadows()
        plan, partials, ticket, sums, trust = self._workspace(C)
        gscale = self._gscale(C)  # (grad_sqnorm first: seg_sqnorm reads its coefficient)
        sched = self._sched_workspace() if self.lr_schedule is not None else None
        C.seg_sqnorm(fs.params, fs.grads, plan, partials, ticket, sums, trust, g["trust_coef"], g["eps"], gscale)
        C.lars(fs.params, fs.grads, self.momentum_buffer, g["lr"], g["momentum"], g["dampening"],
               g["nesterov"], g["maximize"], first, True, shadows, plan, trust, gscale, sched)

    def _grad_torch(self) -> torch.Tensor:
        """The kernels' rule with torch ops: per tensor the norms (summed in float64, rounded
        once) and the fp32 ratio, then lars.hip's element sequence up to the momentum lines."""
        g = self.param_groups[0]
        fs = self.flat
        p, raw = fs.params, fs.grads
        coef = None
        d = raw
        if self.max_grad_norm is not None:
            d = self._clip_torch(raw)
            coef = self._clip_host["coef"]
        d = -d if g["maximize"] else d.clone()
        wds, adapts = self._seg_coefs()
        stats = np.zeros((len(fs.names), 4), dtype=np.float32)
        for s, n in enumerate(fs.names):
            w, gi, di = fs.view(p, n), fs.view(raw, n), fs.view(d, n)
            sw = np.float32(w.double().square().sum().item())
            sg = np.float32(gi.double().square().sum().item())
            wn, gn, ratio = kb.trust_ratio32(sw, sg, wds[s], g["trust_coef"], g["eps"], adapts[s], coef)
            stats[s] = (ratio, wds[s], wn, gn)
            if wds[s] != 0:
                di.add_(w, alpha=float(np.float32(wds[s])))
            di.mul_(float(ratio))
        self._host_stats = stats
        return d

    def trust_stats(self) -> dict | None:
        """Per parameter name ``{"w_norm", "g_norm", "ratio", "adapted"}`` of the last step; on the
        GPU one device-to-host read.  ``None`` before the first step."""
        if self._ws is not None:
            t = self._ws[4][:-1].cpu().numpy()
        elif self._host_stats is not None:
            t = self._host_stats
        else:
            return None
        adapts = self._seg_coefs()[1]
        return {n: {"w_norm": float(t[s, 2]), "g_norm": float(t[s, 3]), "ratio": float(t[s, 0]),
                    "adapted": bool(adapts[s])} for s, n in enumerate(self.flat.names)}

    # ------------------------------------------------------------------ state
    def _group_values(self) -> dict:
        d = super()._group_values()
        if callable(d["exclude"]):
            d["exclude"] = "callable"  # (a function does not belong in a checkpoint: the constructor's is kept)
        return d

    def _load_group(self, saved: dict, keys):
        super()._load_group(saved, [k for k in keys if k != "exclude" or saved.get(k) in (None, "1d")])
        self.hyper_changed()
