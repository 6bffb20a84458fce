"""Exponential moving average of the model's weights, for evaluation and for shipping.

``WeightEMA`` keeps one flat fp32 buffer shaped like ``FlatSpace.params`` and, after every
optimizer step, moves it towards the live parameters:

    e' = e + om * (p - e)          om = fl32(1 - decay_k)

On the GPU that is one HIP kernel (``ema_kernel`` in csrc/kernels/ema.hip), a rule on the
streaming pass the optimizers use: one fp32 subtraction, then one fused multiply-add.  On the CPU
the same subtraction runs in fp32 and the multiply-add in float64, rounded once to fp32 - the
fma's result except where float64's own rounding lands on an fp32 tie.

``warmup=True`` uses ``decay_k = min(decay, (1 + k) / (10 + k))`` for update ``k = 0, 1, ...``
(the rule of ``timm`` / ``tf.train.ExponentialMovingAverage``).  The decay then depends on the
update index, and a captured step graph replays one launch, so nothing that depends on it travels
by value: ``om`` comes from a device-resident table (:func:`warmup_table`) indexed by a device
counter the kernel advances itself - the ``SchedState`` words and ticket protocol ``FusedSGD``
uses for its learning-rate schedule, but a state block of the EMA's own: with ``--grad_accum``
or AdamW the optimizer's counter means something else.  With a constant decay ``om`` is a kernel
argument and the launch only counts itself.

``applied()`` puts the averaged weights in the model's place: ``ema_swap_kernel`` exchanges the
two flat buffers and, in the same pass, rewrites every shadow copy the MFMA kernels read (the
bf16 copy, the PAD4 copies, the optimizer's registered shadows), so every forward and inference
path sees the averaged model.  Leaving the context exchanges them back; an exchange moves bits
and the shadows are functions of the parameters alone, so parameters, shadows, gradients,
BatchNorm buffers and any captured step graph are afterwards as they were, bit for bit.
BatchNorm running statistics are not averaged (``AveragedModel(use_buffers=False)``): the live
ones are used.
"""
from __future__ import annotations

import contextlib
import struct

import torch

from ..models.layers import FlatSpace, flat_space
from .flat_optim import _from_reference_layout, _to_reference_layout

MAX_TABLE = 1 << 22


def _f32(x: float) -> float:
    """``x`` rounded once to float32 (round to nearest even), as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


def warmup_decay(k: int, decay: float) -> float:
    """The decay of update ``k`` with warm-up, in float64."""
    return min(decay, (1 + k) / (10 + k))


def warmup_table(decay: float, max_len: int = MAX_TABLE) -> torch.Tensor:
    """``om_k = fl32(1 - min(decay, (1 + k) / (10 + k)))`` for ``k = 0 .. K``, computed in float64
    and rounded once; ``K`` is the first ``k`` whose warm-up term reaches ``decay``, so the last
    entry is ``fl32(1 - decay)`` and holds for every later update (the reader clamps the index).
    ``ValueError`` if that takes more than ``max_len`` entries."""
    decay = float(decay)
    if not 0.0 < decay < 1.0:
        raise ValueError("decay must lie in (0, 1)")
    est = (10 * decay - 1) / (1 - decay)  # (1 + k) / (10 + k) = decay, solved for k
    if est > max_len + 2:
        raise ValueError(f"decay {decay!r}: the warm-up reaches it after about {est:.3g} updates; the EMA's "
                         f"decay table holds at most {max_len}")
    k = max(0, int(est) - 2)
    while (1 + k) / (10 + k) < decay:
        k += 1
    while k > 0 and k / (9 + k) >= decay:  # (update k - 1 reaches it already)
        k -= 1
    if k + 1 > max_len:
        raise ValueError(f"decay {decay!r}: the warm-up takes {k + 1} updates; the EMA's decay table holds "
                         f"at most {max_len}")
    ks = torch.arange(k + 1, dtype=torch.float64)
    w = torch.clamp((1 + ks) / (10 + ks), max=decay)
    return (1 - w).to(torch.float32)


class WeightEMA:
    """``WeightEMA(model_or_flat, decay=0.9999, warmup=False)``; see the module docstring."""

    def __init__(self, model_or_flat, decay: float = 0.9999, warmup: bool = False):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError("the EMA decay must lie in (0, 1)")
        if isinstance(model_or_flat, FlatSpace):
            self.flat, self.model = model_or_flat, model_or_flat.module
        else:
            self.model, self.flat = model_or_flat, flat_space(model_or_flat)
        self.decay = decay
        self.warmup = bool(warmup)
        self.table = warmup_table(decay) if self.warmup else None  # host float32 [n]
        self.om = _f32(1.0 - decay)
        self.params = self.flat.params.detach().clone()  # (alignment padding: zero there, zero here)
        self._k = 0          # CPU: the number of updates; GPU: the value the state block starts from
        self._ws = None      # GPU: (table or None, state int32[4] = SchedState t / ticket / lr_used)
        self._opt = None     # the optimizer this EMA is attached to (its registered shadows)
        self._applied = False

    # ------------------------------------------------------------------ counter
    def _workspace(self):
        """The decay table (warm-up) and the state words on the device; allocated once, by the
        first update - GraphedStep's warm-up, so before a capture (as ``_clip_workspace``)."""
        if self._ws is None:
            dev = self.params.device
            self._ws = (self.table.to(dev) if self.warmup else None,
                        torch.tensor([self._k, 0, 0, 0], dtype=torch.int32).to(dev))
        return self._ws

    def num_updates(self) -> int:
        """Updates so far; on the GPU one device-to-host read of the counter the kernel advances."""
        if self._ws is not None:
            return int(self._ws[1][0].item())
        return self._k

    def set_num_updates(self, k: int):
        """Continue at update ``k`` (resume).  On the GPU a host-to-device write of the
        counter: never inside a graph capture."""
        k = int(k)
        if k < 0:
            raise ValueError("the number of updates must be >= 0")
        if self._ws is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("set_num_updates inside a graph capture")
            self._ws[1].copy_(torch.tensor([k, 0, 0, 0], dtype=torch.int32))
        self._k = k

    def om_at(self, k: int) -> float:
        """The float32 ``1 - decay_k`` update ``k`` uses."""
        if not self.warmup:
            return self.om
        return self.table[min(max(int(k), 0), self.table.numel() - 1)].item()

    # ------------------------------------------------------------------ API
    @torch.no_grad()
    def reset(self):
        """Start over from the current parameters."""
        self._no_swap("reset")
        self.params.copy_(self.flat.params)
        self.set_num_updates(0)

    @torch.no_grad()
    def update(self):
        """One update from the live parameters; on the GPU one launch on the current stream."""
        self._no_swap("update")
        p = self.flat.params
        if p.is_cuda:
            from .. import native

            table, state = self._workspace()
            native.require().ema(self.params, p, self.om, state, table)
        else:
            om = self.om_at(self._k)
            d = p - self.params
            self.params.copy_((self.params.double() + om * d.double()).float())
            self._k += 1

    def _no_swap(self, what: str):
        if self._applied:
            raise RuntimeError(f"WeightEMA.{what}() inside applied(): the buffers are exchanged")

    def _shadows(self) -> list:
        """Every shadow copy of the model's parameters: the attached optimizer's, else the
        model's bf16 copy and PAD4 copies alone."""
        if self._opt is not None:
            return self._opt._all_shadows()
        fs = self.flat
        if fs._bf16 is None:
            return []
        return [(0, fs.numel, fs._bf16, 1, 0, 0, 0)] + fs.pad4_shadows()

    @torch.no_grad()
    def _swap(self):
        fs = self.flat
        if fs.params.is_cuda:
            from .. import native

            # (the shadows are listed per exchange: a copy first built inside applied() is put
            # back with the rest)
            native.require().ema_swap(fs.params, self.params, self._shadows())
            fs.mark_bf16_fresh()
        else:
            tmp = fs.params.clone()
            fs.params.copy_(self.params)
            self.params.copy_(tmp)

    @contextlib.contextmanager
    def applied(self):
        """Inside, the model is the averaged model (parameters and every shadow copy); after,
        everything is as before, bit for bit.  Not re-entrant."""
        if self._applied:
            raise RuntimeError("WeightEMA.applied() is already active")
        self._swap()
        self._applied = True
        try:
            yield self.model
        finally:
            self._applied = False
            self._swap()

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        """``{"decay", "warmup", "num_updates", "model"}``: ``model`` is a full model state dict
        in the reference layouts (CPU tensors) with the averaged parameters and the live buffers,
        so a plain model loads it with ``model.load_state_dict(sd["model"])``."""
        self._no_swap("state_dict")
        sd = self.model.state_dict()
        avg = _to_reference_layout(self.model, self.flat, self.params)
        out = type(sd)()
        for k, v in sd.items():
            v = avg[k] if k in avg else v
            out[k] = v.detach().to("cpu").clone(memory_format=torch.contiguous_format)
        meta = getattr(sd, "_metadata", None)
        if meta is not None:
            out._metadata = meta
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates(), "model": out}

    @torch.no_grad()
    def load_state_dict(self, sd: dict):
        """Take the averaged parameters and the update count.  ``decay`` and ``warmup`` stay the
        constructor's (the saved ones describe the run that wrote them); the saved buffers are
        the model's own and are not touched here."""
        self._no_swap("load_state_dict")
        ref = {n: sd["model"][n] for n in self.flat.names}
        _from_reference_layout(self.model, self.flat, ref, self.params)
        self.set_num_updates(int(sd["num_updates"]))
