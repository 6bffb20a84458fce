"""A-priori rounding bounds, the error / bound ratio and the CPU replays shared by
tests/test_simplecnn_kernels_elementwise_gpu.py (the HIP kernels) and
tests/test_simplecnn_kernel_bounds_cpu.py (a float32 emulation of a correct kernel, and of
subtly wrong ones).  Nothing here is calibrated on a kernel's output.

u = 2**-24 is the fp32 unit roundoff, n the number of accumulated terms, A the same operation
on absolute values:

    fp32 outputs and slabs      E = 2 n u A          (bf16 operands: exact products)
                                E = 3 n u A          (exact-fp32 builds: the products round too)
    bf16 outputs                2**-8 (|ref| + E) + E

The bf16 store rounds the value the kernel computed, which is within E of the reference, hence
|ref| + E under the 2**-8.
"""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24
BF_EPS = 2.0 ** -8


def acc_bound(n, A, f32_operands=False):
    """fp32 accumulation of n terms whose absolute values sum to A."""
    return (3.0 if f32_operands else 2.0) * n * U * A


def bf16_store_bound(ref, E):
    return BF_EPS * (ref.abs() + E) + E


def ratio(family, shape, out, ref, bound, what, tag="KERN_RATIO"):
    """Prints and returns max |out - ref| / bound; asserts every element written and in bound."""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape, (what, o.shape, ref.shape)
    assert bool(torch.isfinite(o).all()), f"{what}: unwritten / non-finite elements"
    rr = (o - ref).abs() / (bound + 1e-300)
    r = rr.max().item() if rr.numel() else 0.0
    print(f"{tag} {family} {shape} {r:.3e}")
    if r > 1.0:
        i = tuple(int(v) for v in torch.nonzero(rr == rr.max())[0])
        what += f" at {i}: out {o[i].item()!r} ref {ref[i].item()!r}; {int((rr > 1).sum())} elements out of bound"
    assert r <= 1.0, f"{what}: error / bound = {r:.3f}"
    return r


def ratio_value(out, ref, bound):
    """max |out - ref| / bound without asserting (the CPU file's mutation checks)."""
    return ((out.detach().cpu().double() - ref).abs() / (bound + 1e-300)).max().item()


# ------------------------------------------------------------------------------- SGD
def sgd_bounds(p, g, m, lr, momentum, dampening, wd, nesterov, first_step):
    """(bound on the new parameter, bound on the new momentum buffer) of common.h sgd_one.

    sgd_one: d = fma(wd, p, +-g) [1 rounding]; buf = d on the first step, else
    fma(fl(1 - dampening), d, fl(momentum * m)) [3: the product, the difference, the fma];
    d = fma(momentum, buf, d) with nesterov [1]; p' = fma(-lr, d, p) [1].  Each rounding is at
    most u times a partial result that the same formula on absolute values (D1, BUF, D2, P
    below) dominates, and every later step scales it by a factor that formula contains too:
    at most 4 roundings reach the buffer and 6 the parameter.

        |buf' - ref| <= 4 u BUF          |p' - ref| <= 6 u P
    """
    p, g = p.abs(), g.abs()
    D1 = g + abs(wd) * p
    if momentum != 0.0:
        BUF = D1 if first_step else abs(1.0 - dampening) * D1 + abs(momentum) * m.abs()
        D2 = abs(momentum) * BUF + D1 if nesterov else BUF
    else:
        BUF = torch.zeros_like(D1)
        D2 = D1
    P = p + abs(lr) * D2
    return 6 * U * P, 4 * U * BUF


# ----------------------------------------------------------------------- shadow layouts
SHADOW_BF16, SHADOW_BF16_TAPT, SHADOW_BF16_FCFRAG, SHADOW_BF16_PAD4, SHADOW_F32_TAPT, SHADOW_F32_FCFRAG = range(1, 7)


def shadow_index(kind, n, a=0, b=0, c=0):
    """Destination index of every region element j = 0..n-1 (int64 array) - launchers.h:
    plain copy; TAPT: OHWI [co][tap][ci] -> [tap][ci][co] (a = Co, b = taps, c = Ci); FCFRAG:
    [o][hw][c] -> [o][hw/16][c/16][(c/4)%4][hw%16][c%4] (a = HW, b = C); PAD4: [..][3] ->
    [..][4]."""
    j = np.arange(n, dtype=np.int64)
    if kind == SHADOW_BF16:
        return j
    if kind in (SHADOW_BF16_TAPT, SHADOW_F32_TAPT):
        per = b * c
        co = j // per
        return (j - co * per) * a + co
    if kind in (SHADOW_BF16_FCFRAG, SHADOW_F32_FCFRAG):
        HW, C = a, b
        o, rem = j // (HW * C), j % (HW * C)
        hw, ch = rem // C, rem % C
        G, T = HW // 16, C // 16
        return ((((o * G + hw // 16) * T + ch // 16) * 4 + (ch // 4) % 4) * 16 + hw % 16) * 4 + ch % 4
    if kind == SHADOW_BF16_PAD4:
        return (j // 3) * 4 + j % 3
    raise ValueError(kind)


def shadow_dst_numel(kind, n):
    return n // 3 * 4 if kind == SHADOW_BF16_PAD4 else n


def shadow_is_f32(kind):
    return kind in (SHADOW_F32_TAPT, SHADOW_F32_FCFRAG)


# ------------------------------------------------------------- fixed-order slab reduction
def reduce_groups(rows_of_segments):
    """grad_reduce_groups (optim.hip): 16 when the deepest segment has >= 64 rows, else 4."""
    return 16 if max(rows_of_segments) >= 64 else 4


def replay_reduce(rows32, GR):
    """slab_reduce.h's order in float32: group g adds rows g, g + GR, ... sequentially from
    +0.0, the group sums are then added in order 0..GR-1.  rows32: float32 array [rows][n]."""
    rows32 = np.asarray(rows32, dtype=np.float32)
    R, n = rows32.shape
    part = []
    for g in range(GR):
        acc = np.zeros(n, dtype=np.float32)
        for r in range(g, R, GR):
            acc = (acc + rows32[r]).astype(np.float32)
        part.append(acc)
    tot = part[0]
    for g in range(1, GR):
        tot = (tot + part[g]).astype(np.float32)
    return tot


def replay_sequential(rows32):
    rows32 = np.asarray(rows32, dtype=np.float32)
    acc = np.zeros(rows32.shape[1], dtype=np.float32)
    for r in range(rows32.shape[0]):
        acc = (acc + rows32[r]).astype(np.float32)
    return acc


def replay_pairwise(rows32):
    v = [np.asarray(r, dtype=np.float32) for r in rows32]
    while len(v) > 1:
        v = [(v[i] + v[i + 1]).astype(np.float32) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def replay_finish(tot32, scale, prior32=None):
    """The reducer's epilogue on a group total (slab_reduce.h): the float32 product with the
    scale, or with `accum` ONE fma(total, scale, prior).  The fma is evaluated in extended
    precision (the product of two float32 is exact there) and rounded once to float32."""
    s = np.float32(scale)
    tot32 = np.asarray(tot32, dtype=np.float32)
    if prior32 is None:
        return (tot32 * s).astype(np.float32)
    prior32 = np.asarray(prior32, dtype=np.float32)
    return (tot32.astype(np.longdouble) * np.longdouble(s) + prior32.astype(np.longdouble)).astype(np.float32)


def reduce_bound(rows64, scale, prior64=None):
    """|out - scale * sum rows (+ prior)| <= 2 (rows + 2) u (|scale| sum |rows| + |prior|)."""
    R = rows64.shape[0]
    A = abs(scale) * rows64.abs().sum(0)
    if prior64 is not None:
        A = A + prior64.abs()
    return 2 * (R + 2) * U * A


# --------------------------------------------------------------------------- xent_rows
def xent_rows_bounds(x, absum, G, labels, gscale, p, rows):
    """(dlogits bound [B,NO], row-loss bound [B]) of xent_rows (common.h xent_batch_block,
    xent_row_dl) for float64 logits x = bias + the sum of G - 1 partials, absum = |bias| + the
    sum of their absolute values, p the float64 softmax and rows the float64 row losses.

    The logit itself: G fp32 adds, e_l = 2 G u absum (per row: the worst class).  With D =
    max |x - max| the ResNet cross-entropy bound (tests/test_resnet_ops_elementwise_gpu.py)
    takes the argument error u D; here the argument also carries 2 e_l (x and the maximum):

        |dl - ref| <= g (p (2 D + 64) u + 2 p e_l + 2 u)

    The row loss is evaluated as (mx + log se) - x[label]: besides (D + 64) u max(1, |ref|) and
    the two logits' own error 2 e_l, the sum mx + log se and the difference round at the
    logits' magnitude: u (|mx| + log se) + u |ref| <= 2 u (|mx| + |x_label|) + 2 u log se, and
    2 u log se <= 6 u (at most 16 classes) lies inside the constant 64:

        |loss - ref| <= (D + 64) u max(1, |ref|) + 2 e_l + 2 u (|mx| + |x_label|)
    """
    B = x.shape[0]
    e_l = (2 * G * U * absum).max(1).values
    mx = x.max(1).values
    D = (x - mx[:, None]).abs().max(1).values
    bd = gscale * (p * (2 * D[:, None] + 64) * U + 2 * p * e_l[:, None] + 2 * U)
    xl = x[torch.arange(B), labels.long()]
    bl = (D + 64) * U * rows.abs().clamp(min=1.0) + 2 * e_l + 2 * U * (mx.abs() + xl.abs())
    return bd, bl


# ------------------------------------------------------------ global gradient norm (clip)
GN_THREADS, GN_QUADS, GN_MAX_BLOCKS = 256, 4, 1024  # csrc/kernels/launchers.h


def grad_norm_blocks(n):
    """grad_norm_blocks (grad_norm.hip): the grid, a function of n alone."""
    per = GN_THREADS * GN_QUADS
    return int(min(max(((n >> 2) + per - 1) // per, 1), GN_MAX_BLOCKS))


def sqnorm_passes(n):
    """Grid-stride passes of grad_sqnorm_kernel over n elements."""
    per = grad_norm_blocks(n) * GN_THREADS * GN_QUADS
    return ((n >> 2) + per - 1) // per


def _fma32(x32, acc32):
    """float32 fmaf(x, x, acc): the product of two float32 is exact in extended precision,
    the sum is rounded once to float32 (as replay_finish)."""
    x = x32.astype(np.longdouble)
    return (x * x + acc32.astype(np.longdouble)).astype(np.float32)


def _wave_tree(v):
    """wave_sum (common.h) over the last axis (64 lanes): neighbours, then pairs of those, ..."""
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def _block_sum(th):
    """[blocks][256] thread values -> [blocks]: wave trees, then ((w0 + w1) + w2) + w3."""
    w = _wave_tree(th.reshape(th.shape[0], 4, 64))
    return (((w[:, 0] + w[:, 1]).astype(np.float32) + w[:, 2]).astype(np.float32) + w[:, 3]).astype(np.float32)


def replay_sqnorm(g32, n=None, drop=None):
    """The float32 sum of squares of g32[:n] in grad_sqnorm_kernel's documented order
    (csrc/kernels/grad_norm.hip, header).  drop: index of an element left out (the CPU
    tests' mutation)."""
    g32 = np.asarray(g32, dtype=np.float32).reshape(-1)
    n = g32.size if n is None else int(n)
    g32 = g32[:n].copy()
    if drop is not None:
        g32[drop] = 0.0  # fmaf(0, 0, acc) == acc
    G = grad_norm_blocks(n)
    T = G * GN_THREADS
    n4, passes = n >> 2, sqnorm_passes(n)
    quads = np.zeros((max(passes, 1) * GN_QUADS * T, 4), dtype=np.float32)  # skipped quads add +0
    quads[:n4] = g32[:4 * n4].reshape(n4, 4)
    quads = quads.reshape(max(passes, 1), GN_QUADS, T, 4)
    acc = np.zeros((GN_QUADS, T, 4), dtype=np.float32)
    for i in range(passes):
        acc = _fma32(quads[i], acc)
    s = ((acc[..., 0] + acc[..., 1]).astype(np.float32) + (acc[..., 2] + acc[..., 3]).astype(np.float32)).astype(np.float32)
    th = ((s[0] + s[1]).astype(np.float32) + (s[2] + s[3]).astype(np.float32)).astype(np.float32)
    r = n & 3
    if r:
        th[:r] = _fma32(g32[4 * n4:], th[:r])
    part = np.zeros(4 * GN_THREADS, dtype=np.float32)
    part[:G] = _block_sum(th.reshape(G, GN_THREADS))
    p = part.reshape(4, GN_THREADS)
    tj = (((p[0] + p[1]).astype(np.float32) + p[2]).astype(np.float32) + p[3]).astype(np.float32)
    return np.float32(_block_sum(tj.reshape(1, GN_THREADS))[0])


def clip_coef32(norm32, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient in float32: min(1, max_norm / (norm + 1e-6))."""
    q = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return q if np.isnan(q) else np.float32(min(np.float32(1.0), q))


def sqnorm_bound(n, sumsq64):
    """A-priori bounds of grad_sqnorm_kernel for n elements whose squares sum to sumsq64:
    (|S - sum x^2|, |total_norm - sqrt(sum x^2)|, relative error of coef where it is < 1).

    Every term x^2 is non-negative and enters through an fma (the product does not round), so
    with k the longest chain of roundings between a term and S, |S - s| <= gamma_k s,
    gamma_k = k u / (1 - k u).  k = passes (one accumulator's fma chain) + 2 + 2 (the thread's
    16 accumulators) + 1 (tail) + 6 + 3 (wave tree, 4 waves) + 3 + 6 + 3 (the last block over
    the partials) = passes + 26.  sqrtf is correctly rounded: sqrt(s (1 + d)) is within
    sqrt(s) d / 2 (1 + d) of sqrt(s), then one rounding, so the norm's relative error is at most
    e_n = (gamma_k / 2 + u)(1 + gamma_k).  The coefficient adds the rounding of norm + 1e-6f, of
    the constant 1e-6f itself (relative u of a term no larger than the sum) and of the
    division: e_n + 3 u, times (1 + e_n + 3 u) for the reciprocal.
    """
    k = sqnorm_passes(n) + 26
    gk = k * U / (1.0 - k * U)
    e_n = (gk / 2 + U) * (1 + gk)
    e_c = (e_n + 3 * U) * (1 + e_n + 3 * U) / (1 - e_n - 3 * U)
    return gk * sumsq64, e_n * float(np.sqrt(sumsq64)), e_c


# ------------------------------------------------------------ LARS: per-tensor norms, trust ratio
LARS_ITEM, LARS_CHUNK = 4096, 64  # csrc/kernels/launchers.h
LARS_MAX_BLOCKS, LARS_MAX_SEGS = 2048, 4095  # seg_sqnorm_kernel's grid cap; tensors per plan


def lars_items(numel):
    """Work items of a tensor: ceil(numel / LARS_ITEM)."""
    return -(-int(numel) // LARS_ITEM)


def replay_item_partials(rows32):
    """[items][LARS_ITEM] float32 rows (elements at or past an item's len as +0.0f) -> [items]
    partials, steps 1 to 4 of seg_sqnorm_kernel's documented order (csrc/kernels/lars.hip,
    header): per item the 256 threads' folded squares, the wave trees and the block sum."""
    rows32 = np.asarray(rows32, dtype=np.float32).reshape(-1, LARS_ITEM)
    # fmaf(x, x, +0.0f) is the product rounded once: the float32 multiply (and +0.0f for x = -0.0f)
    sq = (rows32 * rows32).reshape(rows32.shape[0], 4, GN_THREADS, 4)  # [item][u][thread][c]
    s = ((sq[..., 0] + sq[..., 1]).astype(np.float32) + (sq[..., 2] + sq[..., 3]).astype(np.float32)).astype(np.float32)
    th = ((s[:, 0] + s[:, 1]).astype(np.float32) + (s[:, 2] + s[:, 3]).astype(np.float32)).astype(np.float32)
    return _block_sum(th)


def replay_seg_finish(part32):
    """One tensor's item partials, in item order -> its sum, step 5 of the same order: lane j's
    sequential sum of the partials j, j + 64, ... from +0.0f, then one more wave tree."""
    lanes = np.zeros(64, dtype=np.float32)
    for k, p in enumerate(np.asarray(part32, dtype=np.float32).reshape(-1)):  # lane k % 64, in item order
        lanes[k % 64] = np.float32(lanes[k % 64] + p)
    return np.float32(_wave_tree(lanes.reshape(1, 64))[0])


def replay_seg_sqnorm(x32):
    """The float32 sum of squares of one tensor's elements x32 in seg_sqnorm_kernel's documented
    order: replay_item_partials over its items, then replay_seg_finish."""
    x32 = np.asarray(x32, dtype=np.float32).reshape(-1)
    k_n = lars_items(x32.size)
    buf = np.zeros(max(k_n, 1) * LARS_ITEM, dtype=np.float32)  # elements past len count as +0.0f
    buf[:x32.size] = x32
    return replay_seg_finish(replay_item_partials(buf)[:k_n])


def seg_sqnorm_chain(numel):
    """Longest chain of roundings between a square and a tensor's sum (lars.hip header)."""
    return 1 + 2 + 2 + 6 + 3 + -(-lars_items(numel) // 64) + 6


def trust_ratio32(sw32, sg32, wd, trust_coef, eps, adapt=True, coef=None):
    """(wn, gn, ratio) in float32 from the float32 sums of squares, as step 6 of
    seg_sqnorm_kernel: correctly rounded roots, gn * coef with clipping, then
    fdiv_rn(trust_coef * wn, fmaf(wd, wn, gn) + eps) if adapt and wn > 0 and gn > 0, else 1."""
    f = np.float32
    wn = f(np.sqrt(np.float64(f(sw32))))
    gn = f(np.sqrt(np.float64(f(sg32))))
    if coef is not None:
        gn = f(gn * f(coef))
    ratio = f(1.0)
    if adapt and wn > 0 and gn > 0:
        den = f(np.longdouble(f(wd)) * np.longdouble(wn) + np.longdouble(gn))  # one fma
        den = f(den + f(eps))
        ratio = f(f(f(trust_coef) * wn) / den)
    return wn, gn, ratio


def trust_ratio_bound(numel, clip=False):
    """A-priori relative bound of the fp32 trust ratio of a tensor of numel elements.

    Each sum of squares has non-negative terms behind a chain of k = seg_sqnorm_chain(numel)
    roundings: relative gamma_k = k u / (1 - k u); the correctly rounded root halves it and adds
    one rounding: e_n = (gamma_k / 2 + u)(1 + gamma_k) per norm (as sqnorm_bound) - half the chain
    length of each norm's summation.  The handful of roundings of the ratio: the numerator's
    product (u); gn's clip multiply (u, with clipping); the denominator's fma and the add of eps
    (2 u; every term is non-negative, so relative errors do not grow); the division (u).  First
    order e_n + u for the numerator, e_n + 3 u for the denominator; second-order terms are
    covered by the factor 1 + 2^-10."""
    k = seg_sqnorm_chain(numel)
    gk = k * U / (1.0 - k * U)
    e_n = (gk / 2 + U) * (1 + gk)
    return (2 * e_n + (6 if clip else 5) * U) * (1 + 2.0 ** -10)


def lars_reference(w, g, m, numels_begins, wds, adapts, lr, momentum, dampening, nesterov, maximize, first,
                   trust_coef, eps, coef=None):
    """The LARS rule (ops/lars.py) in float64 over flat float32 inputs, and the a-priori
    per-element bounds of the fp32 evaluation in lars.hip's order.

    ``numels_begins``: [(begin, numel)] per tensor; ``m``: momentum buffer or None; ``coef``: the
    fp32 clip coefficient or None; every scalar is taken at its float32 value.  Returns
    ``(p64, m64, ratios64, bound_p, bound_m)``; elements outside every tensor keep p and get
    zero bounds.

    Bounds, u = 2^-24, rho_i = trust_ratio_bound of the tensor, first order, each decay / momentum
    multiply-add counted as two roundings (the kernel fuses them into one; the torch path does
    not), magnitudes taken as sums of absolute values:
      d0 = coef g:                   e0 = u |coef g|           (0 without clipping)
      d1 = wd w + d0, A1 = |wd w| + |d0|:   e1 = e0 + 2 u A1   (e0 without decay)
      d2 = d1 R, A2 = R A1:          e2 = R e1 + (rho + u) A2
      buf = d2 (first step): eb = e2, Ab = A2; else buf = (1 - damp) d2 + mom m,
        Ab = (1 - damp) A2 + |mom m|:  eb = (1 - damp) e2 + 3 u (1 - damp) A2 + 2 u |mom m|
        (the fp32 constant 1 - damp, the product, the fma's rounding; mom m and the sum)
      d3 = buf, or with nesterov d2 + mom buf, A3 = A2 + mom Ab:  e3 = e2 + mom eb + 2 u A3
      p' = w - lr d3:                ep = lr e3 + u lr A3 + u (|w| + lr A3)
    both multiplied by 1 + 2^-10 for the second-order terms.  Without momentum d3 = d2."""
    f64 = np.float64
    w64, g64 = np.asarray(w, dtype=np.float32).astype(f64), np.asarray(g, dtype=np.float32).astype(f64)
    m64 = None if m is None else np.asarray(m, dtype=np.float32).astype(f64)
    lr, mom, damp = f64(np.float32(lr)), f64(np.float32(momentum)), f64(np.float32(dampening))
    tc, ep, c = f64(np.float32(trust_coef)), f64(np.float32(eps)), None if coef is None else f64(np.float32(coef))
    p_out, m_out = w64.copy(), (np.zeros_like(w64) if m64 is None else m64.copy())
    bp, bm = np.zeros_like(w64), np.zeros_like(w64)
    ratios = []
    slack = 1 + 2.0 ** -10
    for (b, n), wd, adapt in zip(numels_begins, wds, adapts):
        sl = slice(b, b + n)
        ww, gg = w64[sl], g64[sl]
        wd = f64(np.float32(wd))
        wn, gn = np.sqrt((ww * ww).sum()), np.sqrt((gg * gg).sum())
        if c is not None:
            gn = gn * c
        R = tc * wn / (wd * wn + gn + ep) if (adapt and wn > 0 and gn > 0) else f64(1.0)
        rho = trust_ratio_bound(n, c is not None) if (adapt and wn > 0 and gn > 0) else 0.0
        ratios.append(R)
        d0 = gg if c is None else gg * c
        e0 = 0.0 if c is None else U * np.abs(d0)
        if maximize:
            d0 = -d0
        A1 = np.abs(d0) + np.abs(wd * ww)
        d1 = d0 + wd * ww
        e1 = e0 + (2 * U * A1 if wd != 0 else 0.0)
        d2, A2 = d1 * R, R * A1
        e2 = R * e1 + (rho + U) * A2
        if mom != 0:
            if first:
                buf, eb, Ab = d2, e2, A2
            else:
                mm = mom * m64[sl]
                buf = (1 - damp) * d2 + mm
                Ab = (1 - damp) * A2 + np.abs(mm)
                eb = (1 - damp) * e2 + 3 * U * (1 - damp) * A2 + 2 * U * np.abs(mm)
            m_out[sl], bm[sl] = buf, eb * slack
            if nesterov:
                d3, A3 = d2 + mom * buf, A2 + mom * Ab
                e3 = e2 + mom * eb + 2 * U * A3
            else:
                d3, A3, e3 = buf, Ab, eb
        else:
            d3, A3, e3 = d2, A2, e2
        p_out[sl] = ww - lr * d3
        bp[sl] = (lr * e3 + U * lr * A3 + U * (np.abs(ww) + lr * A3)) * slack
    return p_out, m_out, np.asarray(ratios), bp, bm
