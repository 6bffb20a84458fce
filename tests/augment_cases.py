"""Shared by test_augment_cpu.py and test_augment_gpu.py: the a-priori rounding bound of the
bilinear gather, hand-written parameter rows, and a per-image torch reference (F.pad / slicing
/ flip / F.interpolate) with deliberately wrong variants.

The bound (derived from ddp_amd/data/augment.py's fp32 formulas, nothing fitted).  u = 2**-24,
a box of h x w resampled to H x W, D the largest difference between two horizontally or
vertically adjacent uint8 values of the image's channel, a_c / b_c the affine pair:

* coordinate: s = fl(h / H) is off by <= u h/H; (r + .5) s - .5 therefore by <= u h, and the
  fma rounds once more, <= u h: |ys - ys*| <= 2 u h (the clamp at 0 is 1-Lipschitz), taken as
  E_y = 2 u (h + 1); E_x = 2 u (w + 1) alike.  ly = ys - y0 is exact.
* the interpolant is continuous and piecewise bilinear in (ys, xs) with slopes <= D, ALSO
  across a cell boundary: a coordinate that lands on the other side of an integer in fp32
  picks the neighbouring cell, whose interpolant has the same value on the shared edge, so the
  value moves by <= D (E_y + E_x) whichever cell (int)ys selects.
* the three interpolation fmas and the subtraction b - t each round a value <= 255 once
  (the uint8 differences v01 - v00 are exact): <= 4 u 255.
* the normalising fma: |a_c| times the above, plus u |ref| for its own rounding.
* second-order terms: a factor (1 + 2**-20) on the fp32 part.
* the bf16 store rounds the fp32 value: 2**-8 (|ref| + fp32 error).

    e_val = D (E_y + E_x) + 4 u 255
    e32   = (|a_c| e_val + u |ref|) (1 + 2**-20)
    bound = e32 (1 + 2**-8) + 2**-8 |ref|
"""
import torch
import torch.nn.functional as F

from ddp_amd.data.augment import IMAGENET_MEAN, IMAGENET_STD, affine_table

U = 2.0 ** -24
IMAGENET_AFFINE = affine_table(IMAGENET_MEAN, IMAGENET_STD)
# a second affine with a negative a_c (and one large, one zero offset)
NEG_AFFINE = torch.tensor([[-1.0 / 64, 3.0], [0.0117, -1.5], [1.0 / 255, 0.0]], dtype=torch.float32)
PLAIN_AFFINE = affine_table()


def images(n, H, W, seed=0):
    """uint8 [n, H, W, 3] noise: every neighbour differs, so a misplaced tap shows."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)


def bilinear_bound(images_u8, rows, affine, ref):
    """float64 [B, H, W, 3]: the module docstring's bound for every element of ``ref``."""
    x = images_u8.double()
    D = torch.maximum((x[:, 1:] - x[:, :-1]).abs().amax(dim=(1, 2)) if x.shape[1] > 1 else x.new_zeros(x.shape[0], 3),
                      (x[:, :, 1:] - x[:, :, :-1]).abs().amax(dim=(1, 2)) if x.shape[2] > 1
                      else x.new_zeros(x.shape[0], 3))  # [B, 3]
    rows = rows.double()
    e_coord = 2 * U * (rows[:, 2] + 1) + 2 * U * (rows[:, 3] + 1)  # [B]
    e_val = D * e_coord[:, None] + 4 * U * 255.0
    a = affine.double()[:, 0].abs()
    e32 = ((a * e_val)[:, None, None, :] + U * ref.abs()) * (1 + 2.0 ** -20)
    return e32 * (1 + 2.0 ** -8) + 2.0 ** -8 * ref.abs()


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound over ALL elements (none skipped)."""
    out = out.double()
    assert bool(torch.isfinite(out).all()), "unwritten / non-finite elements"
    return float(((out - ref).abs() / bound).max())


def shift_rows(H, W, P=3):
    """dy, dx in {0, P, 2P} in all nine combinations, each with and without flip: [18, 5]."""
    rows = [(dy - P, dx - P, H, W, f) for f in (0, 1) for dy in (0, P, 2 * P) for dx in (0, P, 2 * P)]
    return torch.tensor(rows, dtype=torch.int32)


def box_rows(H, W):
    """Hand-written boxes of an H x W image, each with and without flip."""
    boxes = [(0, 0, H, W),                                      # the full image
             (0, 0, 1, 1), (0, W - 1, 1, 1), (H - 1, 0, 1, 1), (H - 1, W - 1, 1, 1),  # one pixel per corner
             (H // 2, 0, 1, W), (0, W // 2, H, 1),              # one row, one column
             (1, 2, 2, 2),                                      # 2 x 2 upscaled
             (1, 1, H // 2 + 2, W // 2 + 2)]                    # larger than half the image, downscaled
    return torch.tensor([(*b, f) for f in (0, 1) for b in boxes], dtype=torch.int32)


def torch_reference(img, row, affine, resample, variant=None):
    """One image [H, W, 3] uint8 under one row, float64 [H, W, 3], with torch's own ops.
    ``variant``: None (right) or one of the wrong implementations align_corners / swap_weights /
    flip_first / nearest / pad_after_norm."""
    H, W, _ = img.shape
    top, left, h, w, flip = (int(v) for v in row)
    a, b = affine.double()[:, 0].view(3, 1, 1), affine.double()[:, 1].view(3, 1, 1)
    x = img.permute(2, 0, 1).double()
    if variant == "flip_first" and flip:
        x = x.flip(2)
    if not resample:
        P = max(abs(top), abs(left), 1)
        if variant == "pad_after_norm":
            x = x * a + b
        v = F.pad(x, (P, P, P, P))[:, top + P:top + P + H, left + P:left + P + W]
        if variant == "pad_after_norm":
            a, b = torch.ones_like(a), torch.zeros_like(b)
    else:
        crop = x[:, top:top + h, left:left + w][None]
        if variant == "nearest":
            v = F.interpolate(crop, (H, W), mode="nearest")[0]
        elif variant == "align_corners":
            v = F.interpolate(crop, (H, W), mode="bilinear", align_corners=True)[0]
        elif variant == "swap_weights":
            assert H == W

            def axis(size, out):
                s = ((torch.arange(out).double() + 0.5) * (size / out) - 0.5).clamp_min(0)
                i0 = s.floor().long().clamp_max(size - 1)
                return i0, (i0 + 1).clamp_max(size - 1), s - i0

            (y0, y1, ly), (x0, x1, lx) = axis(h, H), axis(w, W)
            ly, lx = lx.view(1, H, 1), ly.view(1, 1, W)  # <- each weight on the other axis
            c = crop[0]
            t = c[:, y0][:, :, x0] + lx * (c[:, y0][:, :, x1] - c[:, y0][:, :, x0])
            bt = c[:, y1][:, :, x0] + lx * (c[:, y1][:, :, x1] - c[:, y1][:, :, x0])
            v = t + ly * (bt - t)
        else:
            v = F.interpolate(crop, (H, W), mode="bilinear", align_corners=False)[0]
    if flip and variant != "flip_first":
        v = v.flip(2)
    return (v * a + b).permute(1, 2, 0)


def torch_reference_batch(images_u8, rows, affine, resample, variant=None):
    return torch.stack([torch_reference(images_u8[i], rows[i], affine, resample, variant)
                        for i in range(images_u8.shape[0])])


def to_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).double()
