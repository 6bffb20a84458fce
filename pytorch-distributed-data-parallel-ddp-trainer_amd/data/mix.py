"""Mixup and CutMix of the HBM-resident image set, as ``torchvision.transforms.v2.MixUp`` /
``CutMix`` applied after the per-sample transforms: the mixed batch is written by the batch
gather itself (``image_gather_mix_nhwc4``) and the loss trains against a pair target.

All draws are per batch.  Batch row ``b`` is mixed with row ``(b - 1) mod B`` (``x.roll(1, 0)``;
``B`` the actual batch size, a batch of 1 mixes with itself):

* mixup: ``lam ~ Beta(alpha, alpha)``; the row becomes ``lam x[b] + (1 - lam) x[b-1]``.
* cutmix: ``lam0 ~ Beta(alpha, alpha)``, ``cx = randint(W)``, ``cy = randint(H)``,
  ``hw = int(0.5 sqrt(1 - lam0) W)``, ``hh = int(0.5 sqrt(1 - lam0) H)``, the box
  ``x1 = max(cx - hw, 0)``, ``x2 = min(cx + hw, W)`` (the same for y) in OUTPUT coordinates shows
  the partner's pixel, and ``lam = 1 - (x2 - x1)(y2 - y1) / (W H)``.
* the target of either is ``lam t(y[b]) + (1 - lam) t(y[b-1])``, ``t`` the label-smoothed one-hot.

With both alphas a batch picks cutmix with probability ``switch_prob``; with probability
``1 - prob`` it is not mixed at all (``lam = 1``).

The randomness is a pure function of ``(seed, epoch, rank, batch index)``: :meth:`Mix.plan`
draws one record per batch of the epoch from one generator on the host.  The checkpoint gains no
state and a resumed run (which restarts at an epoch boundary) redraws the same records.

The fp32 order every implementation follows (the HIP kernel, :func:`mix_fp32`), with ``n_a`` /
``n_b`` the own / the partner's normalised fp32 value ``fmaf(val, a_c, b_c)`` of augment.py, each
read through its own image's row of the epoch's ``AugPlan``, and ``wa = fp32(lam)``::

    inside the box:  out = bf16(n_b)
    outside it:      out = bf16(n_a)                         if wa == 1
                     out = bf16(fmaf(wa, n_a - n_b, n_b))    otherwise

``wa = fp32(lam)`` and ``wb = fp32(1 - lam)`` are each formed in float64 and rounded once.
"""
from __future__ import annotations

import dataclasses
import math
from typing import NamedTuple

import torch

COLS = 6  # (partner row, x1, y1, x2, y2, bits of the gather's fp32 weight)
NONE, MIXUP, CUTMIX = 0, 1, 2


class PairTarget(NamedTuple):
    """The target of a mixed batch: row b trains against ``w[b, 0] t(y_a[b]) + w[b, 1] t(y_b[b])``.
    ``y_a``, ``y_b`` int64 ``[B]``, ``w`` float32 ``[B, 2]``."""
    y_a: torch.Tensor
    y_b: torch.Tensor
    w: torch.Tensor

    def to(self, *args, **kwargs) -> "PairTarget":
        return PairTarget(*(t.to(*args, **kwargs) for t in self))

    def probs(self, num_classes: int, dtype=torch.float32) -> torch.Tensor:
        """``[B, C]`` class probabilities (before label smoothing)."""
        oh = torch.nn.functional.one_hot
        w = self.w.to(dtype)
        return w[:, 0:1] * oh(self.y_a, num_classes).to(dtype) + w[:, 1:2] * oh(self.y_b, num_classes).to(dtype)


def cutmix_box(lam0: float, cx: int, cy: int, H: int, W: int):
    """``((x1, y1, x2, y2), lam)``: torchvision's box around ``(cx, cy)`` clipped to the image and
    the weight adjusted to the clipped area."""
    r = 0.5 * math.sqrt(1.0 - lam0)
    hw, hh = int(r * W), int(r * H)
    x1, y1, x2, y2 = max(cx - hw, 0), max(cy - hh, 0), min(cx + hw, W), min(cy + hh, H)
    return (x1, y1, x2, y2), 1.0 - float((x2 - x1) * (y2 - y1)) / float(W * H)


def _bits(w32: torch.Tensor) -> torch.Tensor:
    return w32.to(torch.float32).contiguous().view(torch.int32)


def mix_table(partner, box, wa) -> torch.Tensor:
    """The gather's int32 ``[B, 6]`` host table from per-row partners ``[B]``, boxes ``[B, 4]``
    ``(x1, y1, x2, y2)`` and fp32 weights ``[B]``.  A partner outside ``[0, B)`` is refused here,
    before the table reaches a device."""
    partner = torch.as_tensor(partner, dtype=torch.int64).reshape(-1)
    B = partner.numel()
    if B and not bool(((partner >= 0) & (partner < B)).all()):
        raise ValueError(f"mix: partner rows must lie in [0, {B}), got {partner.tolist()}")
    t = torch.empty(B, COLS, dtype=torch.int32)
    t[:, 0] = partner.to(torch.int32)
    t[:, 1:5] = torch.as_tensor(box, dtype=torch.int32).reshape(B, 4)
    t[:, 5] = _bits(torch.as_tensor(wa, dtype=torch.float32).reshape(B))
    return t


@dataclasses.dataclass
class MixPlan:
    """One epoch's host table, one row per batch: ``mode`` int64 ``[steps]`` (NONE / MIXUP /
    CUTMIX), ``box`` int32 ``[steps, 4]`` ``(x1, y1, x2, y2)`` (empty unless cutmix), ``lam``
    float64 ``[steps]`` (the target weight), ``wa`` / ``wb`` float32 ``[steps]``."""
    mode: torch.Tensor
    box: torch.Tensor
    lam: torch.Tensor
    wa: torch.Tensor
    wb: torch.Tensor

    def __len__(self) -> int:
        return self.mode.numel()

    def rows_for(self, step: int, B: int):
        """``(int32 [B, 6] gather table, float32 [B, 2] target weights)`` of batch ``step`` with
        ``B`` rows, on the host.  Only mixup blends in the gather: a cutmix or unmixed batch
        carries the weight 1 there (its pixels are copies)."""
        partner = (torch.arange(B) - 1) % max(B, 1)
        wa_gather = self.wa[step] if int(self.mode[step]) == MIXUP else torch.tensor(1.0)
        table = mix_table(partner, self.box[step].expand(B, 4), wa_gather.expand(B))
        w = torch.stack([self.wa[step], self.wb[step]]).expand(B, 2).contiguous()
        return table, w


class Mix:
    """The mixing recipe; :meth:`plan` turns it into an epoch's table for one rank."""

    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
                 switch_prob: float = 0.5, seed: int = 0):
        if not (mixup_alpha >= 0.0 and cutmix_alpha >= 0.0):  # NaN fails too
            raise ValueError("mixup_alpha and cutmix_alpha must be >= 0 (0 = off)")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError("mix prob and switch_prob must lie in [0, 1]")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.seed = float(prob), float(switch_prob), int(seed)

    @property
    def enabled(self) -> bool:
        return self.mixup_alpha > 0 or self.cutmix_alpha > 0

    def describe(self) -> str:
        parts = ([f"mixup{self.mixup_alpha:g}"] if self.mixup_alpha else []) + \
            ([f"cutmix{self.cutmix_alpha:g}"] if self.cutmix_alpha else [])
        return "+".join(parts)

    def stream_seed(self, epoch: int, rank: int) -> int:
        """The (epoch, rank)'s generator seed: three odd 64-bit multipliers, none of them the
        sampler's ``seed + epoch`` or one of ``Augment.stream_seed``'s."""
        return (0xBF58476D1CE4E5B9 * (self.seed + 1) + 0x94D049BB133111EB * (int(epoch) + 1)
                + 0xDA942042E4DD58B5 * (int(rank) + 1)) % (1 << 63)

    @staticmethod
    def _beta(alpha: float, g: torch.Generator) -> float:
        """Beta(alpha, alpha) as two float64 gamma draws; exactly 0 or 1 can come out at a small
        alpha (both draws underflowing counts as 1)."""
        ga, gb = torch._standard_gamma(torch.full((2,), alpha, dtype=torch.float64), generator=g).tolist()
        return ga / (ga + gb) if ga + gb > 0.0 else 1.0

    def plan(self, epoch: int, rank: int, steps: int, H: int, W: int) -> MixPlan:
        """Records of batches ``0 .. steps - 1``.  Every batch consumes its draws in the same
        order whatever its mode, and the batches are drawn in order from one generator: record
        ``i`` depends on ``(seed, epoch, rank, i)`` only, not on ``steps``, the batch size or the
        world size."""
        g = torch.Generator().manual_seed(self.stream_seed(epoch, rank))
        mode = torch.zeros(steps, dtype=torch.int64)
        box = torch.zeros(steps, 4, dtype=torch.int32)
        lam = torch.ones(steps, dtype=torch.float64)
        for i in range(steps):
            u_apply, u_switch = torch.rand(2, generator=g, dtype=torch.float64).tolist()
            lam_mixup = self._beta(self.mixup_alpha, g) if self.mixup_alpha > 0 else 1.0
            lam_cutmix = self._beta(self.cutmix_alpha, g) if self.cutmix_alpha > 0 else 1.0
            cx = int(torch.randint(W, (1,), generator=g))
            cy = int(torch.randint(H, (1,), generator=g))
            if not self.enabled or not u_apply < self.prob:
                continue
            cut = self.cutmix_alpha > 0 and (self.mixup_alpha <= 0 or u_switch < self.switch_prob)
            if cut:
                b, lam[i] = cutmix_box(lam_cutmix, cx, cy, H, W)
                box[i] = torch.tensor(b, dtype=torch.int32)
                mode[i] = CUTMIX
            else:
                lam[i] = lam_mixup
                mode[i] = MIXUP
        return MixPlan(mode, box, lam, lam.to(torch.float32), (1.0 - lam).to(torch.float32))


def mix_reference(x64: torch.Tensor, y: torch.Tensor, num_classes: int, mode: int, box, lam: float,
                  label_smoothing: float = 0.0):
    """The float64 oracle of one batch: ``x64`` float64 ``[B, H, W, 3]`` (every image after its
    own crop, flip and normalisation), ``y`` int64 ``[B]`` -> (mixed images, target ``[B, C]``),
    with ``roll``, slicing and ``one_hot`` as torchvision writes it.  ``lam`` is the target
    weight (cutmix: the area-adjusted one)."""
    xb = x64.roll(1, 0)
    if mode == MIXUP:
        out = lam * x64 + (1.0 - lam) * xb
    else:
        out = x64.clone()
        if mode == CUTMIX:
            x1, y1, x2, y2 = (int(v) for v in box)
            out[:, y1:y2, x1:x2] = xb[:, y1:y2, x1:x2]
    t = torch.nn.functional.one_hot(y, num_classes).to(torch.float64)
    t = (1.0 - label_smoothing) * t + label_smoothing / num_classes
    return out, lam * t + (1.0 - lam) * t.roll(1, 0)


def mix_fp32(n32: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """What the mixing kernel stores, computed on the host in its fp32 order: ``n32`` float32
    ``[B, H, W, 3]`` unrounded normalised values (``augment.normalized_fp32``), ``table`` int32
    ``[B, 6]`` -> float32 ``[B, H, W, 3]`` holding bf16 values."""
    from .augment import _fma

    table = table.cpu()
    B, H, W, _ = n32.shape
    nb = n32.index_select(0, table[:, 0].to(torch.int64))
    x1, y1, x2, y2 = (table[:, i].view(B, 1, 1) for i in range(1, 5))
    r, c = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    in_box = ((r >= y1) & (r < y2) & (c >= x1) & (c < x2))[..., None]
    wa = table[:, 5].contiguous().view(torch.float32).view(B, 1, 1, 1)
    outside = torch.where(wa == 1.0, n32, _fma(wa.expand_as(n32), n32 - nb, nb))
    return torch.where(in_box, nb, outside).to(torch.bfloat16).float()
