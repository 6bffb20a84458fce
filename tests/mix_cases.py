"""Shared by test_mix_cpu.py and test_mix_gpu.py: hand-written mixing tables, the a-priori
bounds of the mixing gather and of the PAIR cross-entropy kernels, float64 references and a
float32 emulation of the PAIR kernels with deliberately wrong variants.  Everything here runs
on the CPU; nothing is fitted to the kernels.

The mixup pixel bound (u = 2**-24).  n_a, n_b are the fp32 normalised values of the own and the
partner's pixel, each off its float64 value n_a*, n_b* by e_a, e_b: the integer build's single
fma of an exact uint8 value rounds once, e = u |n*|; the bilinear build's e is the fp32 part
e32 of augment_cases.bilinear_bound.  With d* = n_a* - n_b*, lam the float64 weight of the
oracle ref = lam n_a* + (1 - lam) n_b* = n_b* + lam d*, and wa = fp32(lam) <= 1:

* wa is off lam by <= u lam: u lam |d*| in the product;
* d = fl(n_a - n_b) carries e_a + e_b and its own rounding u |d*|, all scaled by wa <= lam (1 + u);
* the fma adds n_b (e_b) and rounds once: u |ref|;
* second-order terms: a factor (1 + 2**-20); the bf16 store: 2**-8 (|ref| + fp32 error).

    e32   = (lam (e_a + e_b + 2 u |d*|) + e_b + u |ref|) (1 + 2**-20)
    bound = e32 (1 + 2**-8) + 2**-8 |ref|

A pixel that is copied (inside the box: the partner's; outside it with wa == 1: the own) is
held to the augmenting gather's own bits, not to a bound.

The PAIR loss bounds extend tests/label_smoothing_cases.bounds (z = x - max, D = max |z|,
A = sum |z|, p the softmax, M = ceil(C / 64)) by the two weighted terms, for the fp32 weights
wa, wb the kernel reads (the float64 reference uses the same fp32 values):

* dlogits: the share keep (ka + kb) rounds twice more (the sum when y_a == y_b, the product):
  2 u on top of the smoothed kernel's 3 u, since wa + wb <= 1 + u:
      bd = gscale (p (2 D + 64) u + 2 u + 5 u)
* loss: each of wa z_a and wb z_b sees the subtraction x - mx, the product, the fma's rounding
  and the product with keep: 4 u each in place of the single label's 3 keep |z_y|:
      bl = mean((D + 64) u max(|row|, 1) + u (4 keep (wa |z_a| + wb |z_b|) + (M + 10) (eps / C) A))
"""
import torch

import augment_cases as AC
import label_smoothing_cases as LS
from ddp_amd.data.mix import mix_table

U = 2.0 ** -24
F32 = torch.float32


def bits_to_f32(col):
    return col.contiguous().view(F32)


# ------------------------------------------------------------------------------- gather cases
def box_cases(H, W):
    """(name, (x1, y1, x2, y2)): empty, full image, one pixel, an edge inside a 4-pixel run at
    each of the four phases (left and right edge), and a box touching each border."""
    cases = [("empty", (0, 0, 0, 0)), ("full", (0, 0, W, H)), ("pixel", (W // 2, H // 2, W // 2 + 1, H // 2 + 1))]
    for ph in range(4):
        x = min(4 * (W // 8) + ph, W - 1)
        cases.append((f"left_edge_phase{ph}", (x, 1, W, H - 1)))
        cases.append((f"right_edge_phase{ph}", (0, 1, max(x, 1), H - 1)))
    cases += [("top", (1, 0, W - 1, 2)), ("bottom", (1, H - 2, W - 1, H)), ("left", (0, 1, 2, H - 1)),
              ("right", (W - 2, 1, W, H - 1))]
    return cases


def table(B, box, wa, partner=None):
    """The int32 [B, 6] table of one batch: every row the same box and weight, partner b - 1."""
    partner = (torch.arange(B) - 1) % B if partner is None else partner
    return mix_table(partner, torch.tensor(box, dtype=torch.int32).expand(B, 4), torch.full((B,), wa, dtype=F32))


def in_box(tab, H, W):
    """bool [B, H, W]: the pixels of each row that lie inside its box."""
    B = tab.shape[0]
    x1, y1, x2, y2 = (tab[:, i].view(B, 1, 1) for i in range(1, 5))
    r, c = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    return (r >= y1) & (r < y2) & (c >= x1) & (c < x2)


def norm_error(images_u8, rows, affine, resample, ref):
    """float64 [B, H, W, 3]: the bound on |n - n*| of the fp32 normalised value (before bf16)."""
    if not resample:
        return U * ref.abs()
    full = AC.bilinear_bound(images_u8, rows, affine, ref)
    return (full - 2.0 ** -8 * ref.abs()) / (1 + 2.0 ** -8)


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound over ALL elements; an element whose bound is 0 (a reference of
    exactly 0 reached without rounding) must be exact."""
    out = out.double()
    assert bool(torch.isfinite(out).all()), "unwritten / non-finite elements"
    return float(((out - ref).abs() / (bound + 1e-300)).max())


def mixup_bound(na, nb, ea, eb, lam):
    """(ref, bound) float64 for own / partner references ``na`` / ``nb`` with fp32 errors
    ``ea`` / ``eb`` and the float64 weight ``lam`` (the module docstring's derivation)."""
    d = na - nb
    ref = nb + lam * d
    e32 = (lam * (ea + eb + 2 * U * d.abs()) + eb + U * ref.abs()) * (1 + 2.0 ** -20)
    return ref, e32 * (1 + 2.0 ** -8) + 2.0 ** -8 * ref.abs()


# --------------------------------------------------------------------------------- loss cases
def pair_inputs(B, C, wa):
    """label_smoothing_cases.xent_inputs (rows offset by 1e4, flat rows, a spread of 60, labels
    on the lane / step boundaries) with a second label per row - equal to the first in every
    third row - and the weights (wa, 1 - wa) rounded to fp32 like MixPlan's."""
    lg, ya = LS.xent_inputs(B, C)
    g = torch.Generator().manual_seed(97 + B + C)
    yb = torch.randint(0, C, (B,), generator=g)
    yb[::3] = ya[::3]
    if B > 1:
        yb[1] = (int(ya[1]) + 64) % C  # the partner in another 64-class step of the same lane
    w = torch.tensor([[wa, 1.0 - wa]], dtype=torch.float64).to(F32).expand(B, 2).contiguous()
    return lg, ya, yb, w


def pair_xent64(lg, ya, yb, w, eps, gscale):
    """float64 (row losses [B], mean loss [1], dlogits [B, C], softmax) for fp32 inputs."""
    x = lg.detach().cpu().double()
    B, C = x.shape
    w = w.detach().cpu().double()
    oh = torch.nn.functional.one_hot
    k = w[:, 0:1] * oh(ya.cpu(), C).double() + w[:, 1:2] * oh(yb.cpu(), C).double()
    t = (1.0 - eps) * k + eps / C
    lsm = torch.log_softmax(x, dim=1)
    rows = -(t * lsm).sum(1)
    return rows, rows.mean().reshape(1), (lsm.exp() - t) * gscale, lsm.exp()


def pair_bounds(lg, ya, yb, w, eps, gscale):
    """(mean loss ref [1], dlogits ref, loss bound [1], dlogits bound): the docstring's bounds."""
    x = lg.detach().cpu().double()
    B, C = x.shape
    M = (C + 63) // 64
    rows, loss_ref, dl_ref, p = pair_xent64(lg, ya, yb, w, eps, gscale)
    z = x - x.max(1, keepdim=True).values
    D, A = z.abs().max(1).values, z.abs().sum(1)
    ar = torch.arange(B)
    w = w.detach().cpu().double()
    za, zb = z[ar, ya.cpu().long()].abs(), z[ar, yb.cpu().long()].abs()
    keep = 1.0 - eps
    bd = gscale * (p * (2 * D[:, None] + 64) * U + 2 * U + 5 * U)
    bl = ((D + 64) * U * rows.abs().clamp(min=1.0)
          + U * (4 * keep * (w[:, 0] * za + w[:, 1] * zb) + (M + 10) * (eps / C) * A)).mean()
    return loss_ref, dl_ref, bl.reshape(1), bd


def emulate_pair(lg, ya, yb, w, eps, gscale, variant="kernel"):
    """The PAIR kernels' arithmetic in float32 in their order (as label_smoothing_cases.emulate).
    ``variant``: ``swapped`` (the weights on the other labels), ``eps_twice`` (eps / C once per
    label: twice in all), ``no_pair`` (the second label ignored)."""
    lg = lg.detach().cpu().to(F32)
    B, C = lg.shape
    M = (C + 63) // 64
    t32 = lambda v: torch.tensor(v, dtype=F32)  # noqa: E731
    eps_t, g = t32(eps), t32(gscale)
    keep, eps_c = t32(1.0) - eps_t, eps_t / t32(float(C))
    if variant == "eps_twice":
        eps_c = eps_c + eps_c
    valid = (torch.arange(64 * M) < C).view(M, 64)
    dl, rows = torch.empty(B, C, dtype=F32), []
    for b in range(B):
        a, bb = int(ya[b]), int(yb[b])
        wa, wb = w[b, 0].to(F32), w[b, 1].to(F32)
        if variant == "swapped":
            wa, wb = wb, wa
        if variant == "no_pair":
            wa, wb = t32(1.0), t32(0.0)
        x = torch.full((64 * M,), float("-inf"), dtype=F32)
        x[:C] = lg[b]
        x = x.view(M, 64)
        mx = lg[b].max()
        z = x - mx
        e = torch.where(valid, torch.exp(z), t32(0.0))
        se_l, sx_l = torch.zeros(64), torch.zeros(64)
        for m in range(M):
            se_l = se_l + e[m]
            sx_l = sx_l + torch.where(valid[m], z[m], t32(0.0))
        se, S = LS._wave_sum(se_l), LS._wave_sum(sx_l)
        zt = LS._fma(wa, lg[b, a] - mx, wb * (lg[b, bb] - mx))
        rows.append(torch.log(se) - (LS._fma(eps_c, S, keep * zt) if eps else zt))
        k = torch.zeros(C, dtype=F32)
        ka, kb = torch.zeros(C, dtype=F32), torch.zeros(C, dtype=F32)
        ka[a], kb[bb] = wa, wb
        k = ka + kb
        pr = (e * (t32(1.0) / se)).view(-1)[:C]
        dl[b] = ((pr - keep * k) - eps_c) * g if eps else (pr - k) * g
    t = t32(0.0)
    for r in rows:
        t = t + r
    return (t / t32(float(B))).reshape(1), dl
