"""Train-time augmentation of the HBM-resident image set: random crop with padding or random
resized crop, horizontal flip, mean/std normalisation - all inside the batch gather.

The randomness is a pure function of ``(seed, epoch, data-set index)``: :meth:`Augment.plan`
draws one row ``(top, left, h, w, flip)`` per data-set image on the host, once per epoch, and
the loader uploads the table next to the epoch's index list.  The checkpoint gains no state, a
resumed run redraws the same table, and an image's augmentation does not depend on the world
size, the batch size or how often the sampler's wrap-around repeats its index.

A row means, for output pixel ``(r, c)`` of an ``H x W`` image:

* integer build (``resample=False``): source pixel ``(r + top, c' + left)`` with
  ``c' = W - 1 - c`` when flipped, else ``c``; ``top`` / ``left`` are ``dy - P`` / ``dx - P`` of
  ``torchvision.transforms.RandomCrop(size, padding=P)`` and may be negative; a source pixel
  outside the image is a black uint8 pixel (0), which then goes through the normalisation like
  any other, because torchvision pads before ``Normalize``; ``h, w`` are ``H, W``.
* bilinear build (``resample=True``): the box ``(top, left, h, w)`` inside the image, drawn by
  ``RandomResizedCrop.get_params``' rule, resampled to ``H x W`` as ``F.interpolate(mode=
  "bilinear", align_corners=False)`` does, then flipped.  The fp32 operation order every
  implementation follows (the HIP kernel, :func:`apply_fp32`)::

      ys = fmaxf(fmaf(r + 0.5f, (float)h / (float)H, -0.5f), 0)
      y0 = min((int)ys, h - 1);  y1 = min(y0 + 1, h - 1);  ly = ys - y0      (the same for x)
      t = fmaf(lx, v01 - v00, v00);  b = fmaf(lx, v11 - v10, v10);  val = fmaf(ly, b - t, t)

Then, in both builds, ``out = bf16(fmaf(val, a_c, b_c))`` with the affine table of
:func:`affine_table`.  :func:`apply_reference` is the float64 oracle of all of it.
"""
from __future__ import annotations

import dataclasses
import math

import torch

COLS = 5  # (top, left, h, w, flip)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def affine_table(mean=None, std=None) -> torch.Tensor:
    """float32 ``[3, 2]`` rows ``(a_c, b_c)``: a uint8 value ``v`` becomes ``fmaf(v, a_c, b_c)``.
    ``a_c = 1 / (255 std_c)``, ``b_c = -mean_c / std_c``, formed in float64 and rounded once;
    without normalisation ``(fp32(1/255), 0)``, the plain gather's ``v * (1.f / 255.f)``."""
    if (mean is None) != (std is None):
        raise ValueError("normalisation needs both mean and std")
    if mean is None:
        mean, std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    m, s = torch.tensor(mean, dtype=torch.float64), torch.tensor(std, dtype=torch.float64)
    if m.shape != (3,) or s.shape != (3,) or not bool((s != 0).all()):
        raise ValueError("mean and std are 3 channel values, std non-zero")
    return torch.stack([1.0 / (255.0 * s), -m / s], dim=1).to(torch.float32).contiguous()


@dataclasses.dataclass
class AugPlan:
    """One epoch's parameter table: ``rows`` int32 ``[n, 5]`` indexed by the data-set index."""
    rows: torch.Tensor
    resample: bool = False

    def to(self, device) -> "AugPlan":
        return AugPlan(self.rows.to(device), self.resample)

    @staticmethod
    def identity(n: int, H: int, W: int, resample: bool = False) -> "AugPlan":
        """No crop, no flip (the bilinear build's identity is the full-image box)."""
        rows = torch.zeros(n, COLS, dtype=torch.int32)
        rows[:, 2], rows[:, 3] = H, W
        return AugPlan(rows, resample)


class Augment:
    """The augmentation recipe; :meth:`plan` turns it into an epoch's table."""

    def __init__(self, crop_pad: int = 0, rrc: bool = False, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                 flip: bool = False, seed: int = 0):
        if crop_pad < 0:
            raise ValueError("crop_pad must be >= 0")
        if crop_pad and rrc:
            raise ValueError("random crop with padding and random resized crop are mutually exclusive")
        if not (0 < scale[0] <= scale[1] <= 1) or not (0 < ratio[0] <= ratio[1]):
            raise ValueError("scale must lie in (0, 1] and ratio be positive, both ascending")
        self.crop_pad, self.rrc, self.flip, self.seed = int(crop_pad), bool(rrc), bool(flip), int(seed)
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))

    @property
    def resample(self) -> bool:
        return self.rrc

    def describe(self) -> str:
        parts = ([f"crop{self.crop_pad}"] if self.crop_pad else []) + (["rrc"] if self.rrc else []) + \
            (["flip"] if self.flip else [])
        return "+".join(parts)

    def stream_seed(self, epoch: int) -> int:
        """The epoch's generator seed: two odd 64-bit multipliers, so it is neither the sampler's
        ``seed + epoch`` nor equal for two (seed, epoch) pairs with the same sum."""
        return (0x9E3779B97F4A7C15 * (self.seed + 1) + 0xD1B54A32D192ED03 * (int(epoch) + 1)) % (1 << 63)

    def plan(self, epoch: int, n: int, H: int, W: int) -> AugPlan:
        """Rows for all ``n`` images of the data set (not the rank's shard) in ``epoch``."""
        if self.crop_pad >= min(H, W):
            raise ValueError(f"crop_pad {self.crop_pad} must be smaller than the image ({H} x {W})")
        g = torch.Generator().manual_seed(self.stream_seed(epoch))
        rows = AugPlan.identity(n, H, W).rows
        if self.crop_pad:
            P = self.crop_pad
            d = torch.randint(0, 2 * P + 1, (n, 2), generator=g)
            rows[:, 0], rows[:, 1] = d[:, 0] - P, d[:, 1] - P
        elif self.rrc:
            rows[:, :4] = self._rrc_boxes(n, H, W, g)
        if self.flip:
            rows[:, 4] = (torch.rand(n, generator=g, dtype=torch.float64) < 0.5).to(torch.int32)
        return AugPlan(rows, self.resample)

    def _rrc_boxes(self, n: int, H: int, W: int, g: torch.Generator) -> torch.Tensor:
        """``RandomResizedCrop.get_params`` for every image at once, in float64: 10 tries of
        (area share, log-uniform aspect), the first whose rounded box fits wins a uniform
        position; else the central crop clamped to the ratio range."""
        tries = 10
        u = torch.rand(n, tries, 2, generator=g, dtype=torch.float64)
        pos = torch.rand(n, 2, generator=g, dtype=torch.float64)
        target = float(H * W) * (self.scale[0] + (self.scale[1] - self.scale[0]) * u[..., 0])
        lr0, lr1 = math.log(self.ratio[0]), math.log(self.ratio[1])
        aspect = torch.exp(lr0 + (lr1 - lr0) * u[..., 1])
        w = torch.round(torch.sqrt(target * aspect)).to(torch.int64)
        h = torch.round(torch.sqrt(target / aspect)).to(torch.int64)
        ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
        first = ok.to(torch.int8).argmax(dim=1, keepdim=True)  # the first fitting try
        found = ok.any(dim=1)
        in_ratio = W / H
        if in_ratio < self.ratio[0]:
            fw, fh = W, int(round(W / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            fh, fw = H, int(round(H * self.ratio[1]))
        else:
            fw, fh = W, H
        fh, fw = min(fh, H), min(fw, W)
        hs = torch.where(found, h.gather(1, first)[:, 0], torch.full((n,), fh))
        ws = torch.where(found, w.gather(1, first)[:, 0], torch.full((n,), fw))
        top = torch.minimum(torch.floor(pos[:, 0] * (H - hs + 1)).to(torch.int64), H - hs)
        left = torch.minimum(torch.floor(pos[:, 1] * (W - ws + 1)).to(torch.int64), W - ws)
        top = torch.where(found, top, (H - hs) // 2)
        left = torch.where(found, left, (W - ws) // 2)
        return torch.stack([top, left, hs, ws], dim=1).to(torch.int32)


def _taps(images_u8: torch.Tensor, yy: torch.Tensor, xx: torch.Tensor) -> torch.Tensor:
    """float64 ``[B, H, W, 3]``: image b at rows ``yy[b]`` ``[B, H]`` and columns ``xx[b]``
    ``[B, W]``; a position outside the image is a black pixel."""
    B, H, W, _ = images_u8.shape
    ok = ((yy >= 0) & (yy < H))[:, :, None] & ((xx >= 0) & (xx < W))[:, None, :]
    b = torch.arange(B)[:, None, None]
    v = images_u8[b, yy.clamp(0, H - 1)[:, :, None], xx.clamp(0, W - 1)[:, None, :]]
    return v.to(torch.float64) * ok[..., None]


def _columns(rows: torch.Tensor, W: int) -> torch.Tensor:
    """int64 ``[B, W]``: the cropped column each output column shows (flip after crop)."""
    c = torch.arange(W)[None, :]
    return torch.where(rows[:, 4:5] != 0, W - 1 - c, c)


def apply_reference(images_u8: torch.Tensor, rows: torch.Tensor, affine: torch.Tensor,
                    resample: bool = False) -> torch.Tensor:
    """The float64 oracle: ``images_u8`` uint8 ``[B, H, W, 3]`` under ``rows`` ``[B, 5]`` (one
    per image of the batch) and ``affine`` ``[3, 2]`` -> float64 ``[B, H, W, 3]``, before the
    bf16 rounding.  Exact arithmetic up to float64 rounding; coordinates as F.interpolate's."""
    images_u8, rows = images_u8.cpu(), rows.cpu().to(torch.int64)
    B, H, W, _ = images_u8.shape
    top, left, h, w = (rows[:, i:i + 1] for i in range(4))
    r, cc = torch.arange(H)[None, :], _columns(rows, W)
    if not resample:
        val = _taps(images_u8, r + top, cc + left)
    else:
        def axis(o, size, out):  # source coordinate, lower tap, upper tap, weight of the upper
            s = ((o.to(torch.float64) + 0.5) * (size.to(torch.float64) / out) - 0.5).clamp_min(0.0)
            i0 = torch.minimum(s.floor().to(torch.int64), size - 1)
            return i0, torch.minimum(i0 + 1, size - 1), s - i0

        y0, y1, ly = axis(r.expand(B, H), h, H)
        x0, x1, lx = axis(cc, w, W)
        ly, lx = ly[:, :, None, None], lx[:, None, :, None]
        v00, v01 = _taps(images_u8, y0 + top, x0 + left), _taps(images_u8, y0 + top, x1 + left)
        v10, v11 = _taps(images_u8, y1 + top, x0 + left), _taps(images_u8, y1 + top, x1 + left)
        t, bt = v00 + lx * (v01 - v00), v10 + lx * (v11 - v10)
        val = t + ly * (bt - t)
    aff = affine.to(torch.float64)
    return val * aff[:, 0] + aff[:, 1]


def _fma(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fp32 fmaf through float64: the product of two fp32 values is exact there."""
    return (a.to(torch.float64) * b.to(torch.float64) + c.to(torch.float64)).to(torch.float32)


def apply_fp32(images_u8: torch.Tensor, rows: torch.Tensor, affine: torch.Tensor,
               resample: bool = False) -> torch.Tensor:
    """What the kernel stores, computed on the host: float32 ``[B, H, W, 3]`` holding bf16
    values.  Integer build: ``v a_c + b_c`` is exact in float64 (an 8-bit by a 24-bit factor
    plus a 24-bit addend of similar magnitude), so ``float64 -> float32 -> bf16`` reproduces the
    kernel's fma and rounding bit for bit.  Bilinear build: the module docstring's fp32
    formulas, operation for operation."""
    return normalized_fp32(images_u8, rows, affine, resample).to(torch.bfloat16).float()


def normalized_fp32(images_u8: torch.Tensor, rows: torch.Tensor, affine: torch.Tensor,
                    resample: bool = False) -> torch.Tensor:
    """:func:`apply_fp32` before its bf16 rounding: the float32 ``fmaf(val, a_c, b_c)`` the kernels
    hold per value (what the mixing gather blends)."""
    if not resample:
        return apply_reference(images_u8, rows, affine, False).to(torch.float32)
    images_u8, rows = images_u8.cpu(), rows.cpu().to(torch.int64)
    B, H, W, _ = images_u8.shape
    top, left, h, w = (rows[:, i:i + 1] for i in range(4))
    f32 = torch.float32

    def axis(o, size, out):
        scale = size.to(f32) / torch.tensor(float(out), dtype=f32)  # IEEE fp32 division
        s = _fma(o.to(f32) + 0.5, scale, torch.tensor(-0.5, dtype=f32)).clamp_min(0.0)
        i0 = torch.minimum(s.to(torch.int64), size - 1)
        return i0, torch.minimum(i0 + 1, size - 1), s - i0.to(f32)

    y0, y1, ly = axis(torch.arange(H)[None, :].expand(B, H), h, H)
    x0, x1, lx = axis(_columns(rows, W), w, W)
    ly, lx = ly[:, :, None, None], lx[:, None, :, None]
    tap = lambda yy, xx: _taps(images_u8, yy + top, xx + left).to(f32)  # noqa: E731
    v00, v01, v10, v11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    t, bt = _fma(lx, v01 - v00, v00), _fma(lx, v11 - v10, v10)
    val = _fma(ly, bt - t, t)
    aff = affine.to(f32)
    return _fma(val, aff[:, 0], aff[:, 1])
