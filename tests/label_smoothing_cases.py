"""Inputs, a-priori bounds and a float32 emulation of the label-smoothed cross-entropy kernels
(xent_wave_rows_kernel<true>, xent_kernel<true>: csrc/kernels/xent_body.h), shared by
tests/test_label_smoothing_cpu.py (whose docstring derives the bounds) and
tests/test_label_smoothing_gpu.py.  Everything here runs on the CPU; nothing is calibrated on
the kernels."""
import math

import torch

from ddp_amd.ops import reference as R

U = 2.0 ** -24
F32 = torch.float32
SHAPES = [(1, 65), (7, 10), (9, 127), (5, 1000)]
EPSILONS = [0.0, 0.1, 0.5, 1.0]


def f32(v: float) -> float:
    """The float32 value a kernel argument of that double becomes (the binding narrows it)."""
    return torch.tensor(v, dtype=F32).item()


def xent_inputs(B, NC):
    """tests/test_resnet_ops_elementwise_gpu.py::xent_inputs on the CPU: rows with an offset of
    1e4, with all logits equal and with a spread of 60, labels forced to the lane / step
    boundaries and the last class."""
    g = torch.Generator().manual_seed(61 + B + NC)
    lg = torch.randn(B, NC, generator=g) * 3
    for i in range(B):
        kind = i % 4
        if kind == 0:
            lg[i] += 1e4
        elif kind == 1:
            lg[i] = 2.5
        elif kind == 2:
            lo, hi = lg[i].min(), lg[i].max()
            lg[i] = (lg[i] - lo) / (hi - lo) * 60.0 - 20
    lab = torch.randint(0, NC, (B,), generator=g)
    forced = [NC - 1, min(64, NC - 1), min(63, NC - 1), 0]
    for i, v in enumerate(forced[:B]):
        lab[i] = v
    return lg, lab


def bounds(lg, lab, eps, gscale):
    """(mean loss ref [1], dlogits ref [B,C], loss bound [1], dlogits bound [B,C]) in float64
    for float32 logits ``lg``; ``eps`` and ``gscale`` are the float32 values the kernel gets."""
    x = lg.detach().cpu().double()
    B, C = x.shape
    M = (C + 63) // 64
    rows, p = R.xent_rows64(lg, lab, eps)
    loss_ref, dl_ref = R.xent64(lg, lab, gscale, eps)
    z = x - x.max(1, keepdim=True).values
    D = z.abs().max(1).values
    A = z.abs().sum(1)
    zy = z[torch.arange(B), lab.cpu().long()].abs()
    keep = 1.0 - eps
    bd = gscale * (p * (2 * D[:, None] + 64) * U + 2 * U + 3 * U)
    bl = ((D + 64) * U * rows.abs().clamp(min=1.0) + U * (3 * keep * zy + (M + 10) * (eps / C) * A)).mean()
    return loss_ref.reshape(1), dl_ref, bl.reshape(1), bd


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).to(F32)


def _wave_sum(v):
    """common.h wave_sum on a [64] float32 vector: the four DPP steps of row16_sum (lane ^ 1,
    lane ^ 2, mirror in each half row, mirror in each row), then (r0 + r1) + (r2 + r3)."""
    lane = torch.arange(64)
    for perm in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
        v = v + v[perm]
    return (v[0] + v[16]) + (v[32] + v[48])


def emulate(lg, lab, eps, gscale, variant="kernel"):
    """The kernels' arithmetic in float32 in their order (lane l owns classes l, l + 64, ...,
    summed per lane in class order, then wave_sum; rows summed in row order); torch's exp / log
    stand in for the fast intrinsics.  Returns (mean loss [1], dlogits [B,C]) as float32.

    ``variant`` names a wrong kernel: ``other_classes`` (eps / (C - 1) over the other classes),
    ``grad_only`` / ``loss_only`` (smoothing in one output only), ``all_slots`` (S over all
    64 M lane slots, the padding's -inf included), ``all_slots_zero`` (the same with a padding
    logit of 0) and ``logit_magnitude`` ((mx + log se) - ... at the logits' own magnitude)."""
    lg = lg.detach().cpu().to(F32)
    B, C = lg.shape
    M = (C + 63) // 64
    t32 = lambda v: torch.tensor(v, dtype=F32)  # noqa: E731
    eps_t, g = t32(eps), t32(gscale)
    keep = t32(1.0) - eps_t
    eps_c = eps_t / t32(float(C))
    eps_o = eps_t / t32(float(max(C - 1, 1)))
    valid = (torch.arange(64 * M) < C).view(M, 64)
    dl = torch.empty(B, C, dtype=F32)
    rows = []
    for b in range(B):
        y = int(lab[b])
        pad = 0.0 if variant == "all_slots_zero" else -math.inf
        x = torch.full((64 * M,), pad, dtype=F32)
        x[:C] = lg[b]
        x = x.view(M, 64)
        mx = lg[b].max()
        z = x - mx
        e = torch.where(valid, torch.exp(z), t32(0.0))
        se_l, sx_l, sr_l = torch.zeros(64), torch.zeros(64), torch.zeros(64)
        every = variant in ("all_slots", "all_slots_zero")
        for m in range(M):
            se_l = se_l + e[m]
            sx_l = sx_l + (z[m] if every else torch.where(valid[m], z[m], t32(0.0)))
            sr_l = sr_l + torch.where(valid[m], x[m], t32(0.0))
        se, S, SR = _wave_sum(se_l), _wave_sum(sx_l), _wave_sum(sr_l)
        xl = lg[b, y]
        zl = xl - mx
        lse = torch.log(se)
        if variant == "grad_only":
            row = lse - zl
        elif variant == "other_classes":
            row = lse - _fma(eps_o, S - zl, keep * zl)
        elif variant == "logit_magnitude":
            row = (mx + lse) - _fma(eps_c, SR, keep * xl)
        else:
            row = lse - _fma(eps_c, S, keep * zl)
        rows.append(row)
        inv = t32(1.0) / se
        onehot = torch.zeros(C, dtype=F32)
        onehot[y] = 1.0
        pr = (e * inv).view(-1)[:C]
        if variant == "loss_only":
            dl[b] = (pr - onehot) * g
        elif variant == "other_classes":
            dl[b] = ((pr - keep * onehot) - eps_o * (1 - onehot)) * g
        else:
            dl[b] = ((pr - keep * onehot) - eps_c) * g
    t = t32(0.0)
    for r in rows:
        t = t + r
    return (t / t32(float(B))).reshape(1), dl


def within(out, ref, bound):
    """Every element finite and |out - ref| <= bound; returns (ok, max error / bound)."""
    o = out.detach().cpu().double()
    if not bool(torch.isfinite(o).all()):
        return False, math.inf
    r = ((o - ref).abs() / (bound + 1e-30)).max().item()
    return r <= 1.0, r
