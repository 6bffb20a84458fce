"""ResNet BatchNorm, pooling, cross-entropy and head-GEMM kernels per element, on MI355X.

Every kernel of csrc/kernels/resnet_ops.hip that is not a convolution (and the block
cross-entropy of xent.hip) is compared with the float64 CPU reference of the same operation
(ddp_amd/ops/reference.py, itself held against torch's double-precision operators by
tests/test_resnet_ops_reference_cpu.py) on the same inputs, element by element, against an
a-priori rounding bound.  Nothing is calibrated on the kernels.  u = 2**-24 (fp32 unit
roundoff); 2**-8 |ref| is the one bf16 rounding of a stored bf16 output.

BatchNorm apply (bn_affine.h + bn_apply_kernel): sc = fl(invstd * gamma) [1 rounding],
sh = fma(-mean, sc, beta) [1], v = fma(x, sc, sh) [1], v + res [1], ReLU exact, one bf16
store.  Each rounding is at most u times a partial result no larger than
|x sc| + |mean sc| + |beta| + |res|, so

    |y - ref| <= 2**-8 |ref| + 4 u (|x sc| + |mean sc| + |beta| + |res|)

BatchNorm backward: d = bf16(d1 + d2) (fp32 add, bf16 store - reproduced exactly on the
CPU), masked by out > 0 on the tensor bn_apply stored.  dres is d itself: bit for bit.
sum d: P exact bf16 terms added in fp32 in some order, re-summed over lanes / rows (factor 2):

    |sums[:C] - S_d| <= 2 P u sum|d|                       =: E_d

sum d * xhat: xhat = fl(fl(x - mean) * invstd) [2 roundings], the fma's product is exact, its
add rounds once per term like any summation step, re-summed (factor 2):

    |sums[C:] - S_q| <= 2 (P + 3) u sum|d xhat|             =: E_q

dgamma / dbeta are the same values (bitwise); `accum` adds the prior as one more term (one
fp32 add, also checked bitwise).  dx = k (count d - S_d - xhat S_q), k = fl(fl(gamma invstd)
/ count) [2], count d [1], - S_d [1], xhat [2], xhat S_q [1], the subtraction [1], k * [1] -
at most 6 roundings on any one path, each at most u times count|d| + |S_d| + |xhat S_q| -
plus the kernel's own sums instead of the float64 ones, plus the bf16 store:

    |dx - ref| <= 2**-8 |ref| + |k| [6 u (count |d| + |S_d| + |xhat S_q|) + E_d + |xhat| E_q]

Max pool: the maximum of bf16 values and its first position are exact: y and argmax equal
the reference bit for bit / element for element.  The backward sums at most 4 routed
d = bf16(dy + dy2) in fp32 in window order kh, kw and stores bf16: reproduced in float32 on
the CPU in that order and compared bit for bit, and within 2**-8 |ref| of the float64 sum.

Average pool: HW exact terms summed in fp32 (32 lanes, then the lanes: factor 2) and one
division: |y - ref| <= 2 (HW + 1) u sum|x| / HW.  Backward: one fp32 division and one bf16
store: 2**-8 |ref| + 2 u |ref|.

Head GEMMs (fp32 out): K exact-product fma steps per K slice (or MFMA steps: products of
fp32 operands rounded, hence 2 K), the slices re-summed, alpha, bias, prior [3]:

    |out - ref| <= 2 (2 K + 3) u (|alpha| |A| |B| + |bias| + |prior|)

Cross-entropy: with p the float64 softmax, D = max |x - max| of the row and g = gscale,

    |dlogits - ref| <= g (p (2 D + 64) u + 2 u)
    |loss - ref|    <= mean over rows of (D + 64) u max(1, |ref_row|)

x - max is exact up to u D; the fast exp (v_exp_f32 on x * log2 e) carries the argument's
rounding u D into a relative error, twice (numerator and the sum); the constant 64 covers
the intrinsics' own error (1 ulp each), the 16-step lane sum, the wave reduction and 1 / sum.
The absolute term is 2 u, not the single u one rounding would give: after p the kernel
rounds twice more, (p - onehot) and the product with g, each up to u relative to a value
that is 1 at a label with small p (g = 1/7, p -> 0: 2**-25 g from the subtraction plus half
an ulp of 0.1428 = 2**-27 from the product is 1.37 g u - exact float32 arithmetic of the
formula itself breaks a bound of g u; reproduced on the CPU at (7, 10)).  g is the float32
value the kernel receives (the binding narrows the double), in the reference too.

Every output and workspace is carved out of a larger buffer with sentinel bands on both
sides (nothing outside is written) and pre-filled with NaN (every element is written).
Run with -s for the OPS_RATIO <family> <shape> <error / bound> lines;
profiles/resnet_ops/README.md records the largest per family and shape.
"""
import pytest
import torch

from ddp_amd.ops import reference as R
from elementwise import BF, F32, Guarded, U, bits, f64, report_ratio, rnd

pytestmark = pytest.mark.gpu
dev = "cuda"
BN_BWD_PX_DEFAULT = 392  # resnet_ops.hip g_bn_bwd_px


def ratio(family, shape, out, ref, bound, what):
    """Prints and returns max |out - ref| / bound; asserts every element written and in bound."""
    o = f64(out)
    assert o.shape == ref.shape, (what, o.shape, ref.shape)
    assert bool(torch.isfinite(o).all()), f"{what}: unwritten / non-finite elements"
    rr = (o - ref).abs() / (bound + 1e-30)
    r = rr.max().item()
    report_ratio(r, family, shape, tag="OPS_RATIO")
    if r > 1.0:
        i = tuple(int(v) for v in torch.nonzero(rr == rr.max())[0])
        what += f" at {i}: out {o[i].item()!r} ref {ref[i].item()!r}; {int((rr > 1).sum())} elements out of bound"
    assert r <= 1.0, f"{what}: error / bound = {r:.3f}"
    return r


def bn_params(Cc, seed):
    g = torch.Generator().manual_seed(seed)
    mean = (torch.randn(Cc, generator=g) * 0.1).to(dev)
    invstd = (torch.rand(Cc, generator=g) + 0.5).to(dev)
    gamma = (torch.rand(Cc, generator=g) + 0.5).to(dev)
    beta = (torch.randn(Cc, generator=g) * 0.3).to(dev)
    return mean, invstd, gamma, beta


# ------------------------------------------------------------------------- BatchNorm apply
@pytest.mark.parametrize("res,relu", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("N,H,W,Cc", [(3, 13, 13, 64), (2, 25, 25, 128), (5, 7, 7, 512), (1, 3, 3, 64),
                                      (2, 4, 4, 256)])
def test_bn_apply(C, N, H, W, Cc, res, relu):
    x = rnd(N, H, W, Cc, seed=1)
    r = rnd(N, H, W, Cc, seed=2) if res else None
    mean, invstd, gamma, beta = bn_params(Cc, 3)
    y = Guarded((N, H, W, Cc), BF)
    C.bn_apply(x, mean, invstd, gamma, beta, r, relu, y.t)
    torch.cuda.synchronize()
    ref = R.bn_apply64(x, mean, invstd, gamma, beta, r, relu)
    sc = f64(invstd) * f64(gamma)
    mag = (f64(x) * sc).abs() + (f64(mean) * sc).abs() + f64(beta).abs() + (f64(r).abs() if res else 0.0)
    what = f"bn_apply {(N, H, W, Cc)} res={res} relu={relu}"
    ratio("bn_apply", (N, H, W, Cc), y.t, ref, 2.0 ** -8 * ref.abs() + 4 * U * mag, what)
    if relu:
        assert bool((f64(y.t) >= 0).all())
    y.check(what)


# ------------------------------------------------------------------------ BatchNorm backward
# (px per block, P, C)
BN_BWD_CASES = [
    (392, 9, 64), (392, 32, 64), (392, 245, 64), (392, 507, 64),
    (392, 1250, 128),                        # two strips, two tickets
    (160, 480, 64), (160, 700, 64),          # rpb between 128 and 255: n4 in {0, 1, 2}, both short tails
    (32, 1000, 64),                          # R = 31, rpb = 33, last block 10 pixels: idle lanes
    (32, 1900, 64),                          # R = 58: only phases 0 and 1 take the 8-in-flight row loop
    (32, 2101, 64),                          # R = 64: every phase takes it once
    (32, 3200, 64),                          # R = 100: the 8-in-flight loop and the one-row loop
    (32, 8200, 64),                          # R = 249: three 8-in-flight rounds, phase 0 a fourth
    (32, 8192, 64),                          # R = 256, the cap
]


def launch_rule(P, px):
    """resnet_ops.hip bn_bwd_rows: (rows of the grid, pixels per block)."""
    R_ = min(max(P // px, 1), 256)
    rpb = -(-P // R_)
    return -(-P // rpb), rpb


def lane_paths(P, px):
    """Per block and pixel lane of bn_bwd_reduce_kernel: (n4, two-pixel tail iterations,
    one-pixel tail iterations, idle)."""
    rows, rpb = launch_rule(P, px)
    out = []
    for y in range(rows):
        p0, p1 = y * rpb, min(P, (y + 1) * rpb)
        for tp in range(32):
            p = p0 + tp
            n4 = (p1 - p - 96 + 127) // 128 if p1 - p - 96 > 0 else 0
            q = p + 128 * n4
            t2 = 0
            while q + 32 < p1:
                q += 64
                t2 += 1
            t1 = 0
            while q < p1:
                q += 32
                t1 += 1
            assert (4 * n4 + 2 * t2 + t1) == len(range(p, p1, 32))  # every pixel of the lane, once
            out.append((n4, t2, t1, p >= p1))
    return rows, rpb, out


def test_bn_bwd_cases_cover_every_path():
    """The case table reaches every stage of the reduce kernel's pixel loop and of its
    last-arrival row loop - computed from the launch rule, so the table cannot rot."""
    n4s, t2s, t1s, idle, Rs = set(), set(), set(), False, set()
    for px, P, Cc in BN_BWD_CASES:
        rows, rpb, lanes = lane_paths(P, px)
        Rs.add(rows)
        for n4, t2, t1, idl in lanes:
            n4s.add(min(n4, 4))
            t2s.add(t2 > 0)
            t1s.add(t1 > 0)
            idle |= idl
    assert n4s == {0, 1, 2, 3, 4}, n4s
    assert t2s == {False, True} and t1s == {False, True} and idle
    assert 1 in Rs and 256 in Rs
    assert any(1 < r < 8 for r in Rs) and any(57 <= r <= 64 for r in Rs) and any(64 < r < 256 for r in Rs)
    # a partial 8-in-flight round (some phases in it, some not) and a full one
    assert any(57 <= r < 64 for r in Rs) and 64 in Rs


@pytest.fixture
def bn_bwd_px(C):
    def set_px(px):
        C.bn_bwd_set_px_per_block(px)
    try:
        yield set_px
    finally:
        C.bn_bwd_set_px_per_block(BN_BWD_PX_DEFAULT)


class BnBwdCase:
    """Inputs of one BatchNorm backward geometry and the saved outputs bn_apply stores."""

    def __init__(self, C, P, Cc):
        self.shape = (1, P, 1, Cc)
        self.x = rnd(*self.shape, seed=11)
        self.mean, self.invstd, self.gamma, self.beta = bn_params(Cc, 12)
        # channel 0: x == mean and beta == 0: the BN output is exactly 0 (the mask's edge)
        self.mean[0] = 0.25
        self.beta[0] = 0.0
        self.x[..., 0] = 0.25
        self.d1 = rnd(*self.shape, seed=13)
        self.d2 = rnd(*self.shape, seed=14)
        self.res = rnd(*self.shape, seed=15)
        self.out_plain = torch.empty_like(self.x)  # BatchNorm + ReLU (mask_beta recomputes its sign)
        C.bn_apply(self.x, self.mean, self.invstd, self.gamma, self.beta, None, True, self.out_plain)
        self.out_res = torch.empty_like(self.x)    # BatchNorm + residual + ReLU
        C.bn_apply(self.x, self.mean, self.invstd, self.gamma, self.beta, self.res, True, self.out_res)
        torch.cuda.synchronize()
        assert bool((self.out_plain[..., 0] == 0).all()) and bool((self.out_plain > 0).any())
        self.ref = {}

    def reference(self, mask, two):
        """d (bf16 exact, float64) and the float64 backward of it - once per (mask, dout2)."""
        if (mask, two) not in self.ref:
            d = (self.d1.float() + self.d2.float()).to(BF) if two else self.d1
            d = f64(d)
            keep = None
            if mask == "out":
                keep = f64(self.out_res) > 0
            elif mask == "beta":
                keep = f64(self.out_plain) > 0
            if keep is not None:
                d = torch.where(keep, d, torch.zeros_like(d))
            P = self.shape[1]
            self.ref[(mask, two)] = (d, keep, R.bn_bwd64(d, self.x, self.mean, self.invstd, self.gamma, float(P)))
        return self.ref[(mask, two)]


_BN_CASES = {}


@pytest.mark.parametrize("mask", ["none", "out", "beta"])
@pytest.mark.parametrize("px,P,Cc", BN_BWD_CASES)
def test_bn_bwd(C, bn_bwd_px, px, P, Cc, mask):
    """Every mask mode at every geometry, each with dout2 absent / present and accum off / on."""
    bn_bwd_px(px)
    rows, rpb = launch_rule(P, px)
    assert C.bn_bwd_rows(P, Cc) == rows, (P, px, rows)
    if (P, Cc) not in _BN_CASES:
        _BN_CASES[(P, Cc)] = BnBwdCase(C, P, Cc)
    cs = _BN_CASES[(P, Cc)]
    g = torch.Generator().manual_seed(17)
    prior_g, prior_b = torch.randn(Cc, generator=g).to(dev), torch.randn(Cc, generator=g).to(dev)
    for two in (False, True):
        for accum in (False, True):
            what = f"bn_bwd P={P} C={Cc} px={px} R={rows} rpb={rpb} mask={mask} dout2={two} accum={accum}"
            shape = (px, P, Cc)
            d, keep, ref = cs.reference(mask, two)
            ws = Guarded((rows, 2, Cc), F32)
            sums, dg, db = Guarded((2 * Cc,), F32), Guarded((Cc,), F32), Guarded((Cc,), F32)
            dx, dres = Guarded(cs.shape, BF), Guarded(cs.shape, BF)
            if accum:
                dg.t.copy_(prior_g)
                db.t.copy_(prior_b)
            args = (cs.d1, cs.out_res if mask == "out" else None, cs.x, cs.mean, cs.invstd, cs.gamma, float(P))
            tail = (cs.d2 if two else None, cs.beta if mask == "beta" else None)
            C.bn_bwd(*args, ws.t, sums.t, dg.t, db.t, accum, dx.t, dres.t, *tail)
            torch.cuda.synchronize()
            for g_ in (ws, sums, dg, db, dx, dres):
                g_.check(what)
            assert bool(torch.isfinite(ws.t).all()), f"{what}: unwritten workspace rows"
            # dres: the masked upstream gradient itself
            assert torch.equal(f64(dres.t), d), f"{what}: dres != d"
            if keep is not None:
                assert bool((f64(dres.t)[~keep] == 0).all())
            # the two channel sums
            E_d = 2 * P * U * ref["abs_d"]
            E_q = 2 * (P + 3) * U * ref["abs_dxh"]
            ratio("bn_bwd_sum_d", shape, sums.t[:Cc], ref["sum_d"], E_d, what)
            ratio("bn_bwd_sum_dxh", shape, sums.t[Cc:], ref["sum_dxh"], E_q, what)
            # dgamma / dbeta
            if accum:
                pg, pb = f64(prior_g), f64(prior_b)
                ratio("bn_bwd_dgamma_accum", shape, dg.t, pg + ref["sum_dxh"],
                      2 * (P + 4) * U * (ref["abs_dxh"] + pg.abs()), what)
                ratio("bn_bwd_dbeta_accum", shape, db.t, pb + ref["sum_d"],
                      2 * (P + 1) * U * (ref["abs_d"] + pb.abs()), what)
                assert torch.equal(bits(dg.t), bits(prior_g + sums.t[Cc:]))  # one fp32 add of the prior
                assert torch.equal(bits(db.t), bits(prior_b + sums.t[:Cc]))
            else:
                assert torch.equal(bits(dg.t), bits(sums.t[Cc:])) and torch.equal(bits(db.t), bits(sums.t[:Cc]))
            # dx against the float64 sums
            k = (f64(cs.gamma) * f64(cs.invstd) / P).abs()
            xh = ref["xh"].abs()
            bound = 2.0 ** -8 * ref["dx"].abs() + k * (
                6 * U * (P * d.abs() + ref["sum_d"].abs() + xh * ref["sum_dxh"].abs()) + E_d + xh * E_q)
            ratio("bn_bwd_dx", shape, dx.t, ref["dx"], bound, what)
            # fixed-order reductions: a second call is bitwise identical
            ws2 = Guarded((rows, 2, Cc), F32)
            sums2, dx2 = Guarded((2 * Cc,), F32), Guarded(cs.shape, BF)
            C.bn_bwd(*args, ws2.t, sums2.t, None, None, False, dx2.t, None, *tail)
            torch.cuda.synchronize()
            assert torch.equal(bits(sums.t), bits(sums2.t)) and torch.equal(bits(dx.t), bits(dx2.t)), what
            for g_ in (ws2, sums2, dx2):
                g_.check(what)


# ------------------------------------------------------------------------------- max pool
POOL_SHAPES = [(2, 1, 1, 64), (2, 2, 2, 64), (3, 3, 5, 24), (2, 8, 11, 64), (2, 9, 9, 64), (1, 25, 25, 64),
               (2, 7, 4, 8)]


def pool_input(kind, shape):
    g = torch.Generator().manual_seed(21)
    t = torch.randn(*shape, generator=g)
    if kind == "relu":
        t = torch.relu(t)                            # zeros: ties in most windows
    else:
        t = (t * 2).round().clamp(-2, 2) / 2 + 0.0   # multiples of 0.5 in [-1, 1]; no -0
    return t.to(BF).to(dev)


@pytest.mark.parametrize("kind", ["relu", "quantised"])
@pytest.mark.parametrize("N,H,W,Cc", POOL_SHAPES)
def test_maxpool_fwd_bwd(C, N, H, W, Cc, kind):
    x = pool_input(kind, (N, H, W, Cc))
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y, am = Guarded((N, OH, OW, Cc), BF), Guarded((N, OH, OW, Cc), torch.uint8)
    C.maxpool_fwd(x, y.t, am.t)
    torch.cuda.synchronize()
    what = f"maxpool {(N, H, W, Cc)} {kind}"
    y_ref, idx, bwd = R.maxpool64(x)
    assert torch.equal(bits(y.t), bits(y_ref.to(BF))), f"{what}: y"
    got = am.t.cpu().long()
    assert int(got.max()) <= 8, f"{what}: unwritten argmax"
    bad = int((got != idx).sum())
    print(f"OPS_RATIO maxpool_argmax_mismatches {(N, H, W, Cc)} {bad}")
    assert bad == 0, f"{what}: {bad} argmax elements differ from the first maximum"
    y.check(what)
    am.check(what)
    dy, dy2 = rnd(N, OH, OW, Cc, seed=22), rnd(N, OH, OW, Cc, seed=23)
    for two in (False, True):
        dx = Guarded((N, H, W, Cc), BF)
        C.maxpool_bwd(dy, am.t, dx.t, dy2 if two else None)
        torch.cuda.synchronize()
        d = (dy.float() + dy2.float()).to(BF) if two else dy
        want32 = bwd(d.float(), torch.float32).to(BF)  # fp32 sum in window order, one bf16 rounding
        assert bool(torch.isfinite(dx.t).all()), f"{what}: unwritten dx"
        assert torch.equal(bits(dx.t), bits(want32)), f"{what}: dx (dy2={two})"
        ref = bwd(d)
        ratio("maxpool_bwd", (N, H, W, Cc), dx.t, ref, 2.0 ** -8 * ref.abs(), what)
        dx.check(what)


# ---------------------------------------------------------------------------- average pool
@pytest.mark.parametrize("Cc", [64, 512])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 3), (4, 4), (1, 31), (4, 8), (3, 11), (7, 7), (9, 9)])
def test_avgpool_fwd_bwd(C, H, W, Cc):
    N, HW = 3, H * W
    x = rnd(N, H, W, Cc, seed=31, relu=True)
    x[0] = rnd(H, W, Cc, seed=32)  # one signed image
    y = Guarded((N, Cc), F32)
    C.avgpool_fwd(x, y.t)
    torch.cuda.synchronize()
    what = f"avgpool HW={HW} C={Cc}"
    A = f64(x).abs().reshape(N, HW, Cc).sum(1)
    ratio("avgpool_fwd", (N, HW, Cc), y.t, R.avgpool64(x), 2 * (HW + 1) * U * A / HW, what)
    y.check(what)
    dy = rnd(N, Cc, seed=33, dtype=F32)
    dx = Guarded((N, H, W, Cc), BF)
    C.avgpool_bwd(dy, dx.t)
    torch.cuda.synchronize()
    ref = R.avgpool_bwd64(dy, H, W)
    ratio("avgpool_bwd", (N, HW, Cc), dx.t, ref, (2.0 ** -8 + 2 * U) * ref.abs(), what)
    dx.check(what)


# ------------------------------------------------------------------------------ head GEMMs
def run_gemm(C, M, N, K, a_bf16=False, b_bf16=False, alpha=1.0, accum=False, bias=True, a_layout="mk",
             b_kn=False):
    """One C.sgemm call; A as [M,K] ("mk"), stored transposed [K,M] ("km": sam = 1, sak = M) or
    a ones row read with sam = 0 ("ones"); B as a weight [N,K] or, b_kn, as [K,N]."""
    small = M <= 32 and K >= 64  # resnet_ops.hip sgemm(): the MFMA small-M kernel
    ta, tb = (BF if a_bf16 else F32), (BF if b_bf16 else F32)
    if a_layout == "ones":
        assert M == 1
        A = torch.ones(K, dtype=ta, device=dev)
        A2, sam, sak = A.view(1, K), 0, 1
    elif a_layout == "km":
        A = rnd(K, M, seed=41, dtype=ta)
        A2, sam, sak = A.t(), 1, M
    else:
        A = rnd(M, K, seed=41, dtype=ta)
        A2, sam, sak = A, K, 1
    if b_kn:
        Bm = rnd(K, N, seed=42, dtype=tb)
        B2, sbk, sbn = Bm, N, 1
    else:
        Bm = rnd(N, K, seed=42, dtype=tb)
        B2, sbk, sbn = Bm.t(), 1, K
    bv = rnd(N, seed=43, dtype=F32) if bias else None
    prior = rnd(M, N, seed=44, dtype=F32) if accum else None
    out = Guarded((M, N), F32)
    if accum:
        out.t.copy_(prior)
    C.sgemm(M, N, K, A, sam, sak, Bm, sbk, sbn, out.t, bv, alpha, accum)
    torch.cuda.synchronize()
    what = (f"sgemm {(M, N, K)} a_bf16={a_bf16} b_bf16={b_bf16} alpha={alpha} accum={accum} bias={bias} "
            f"A={a_layout} b_kn={b_kn}")
    ref = R.gemm64(A2, B2, bv, alpha, prior)
    mag = R.gemm64(f64(A2).abs(), f64(B2).abs(), None if bv is None else bv.abs(), abs(alpha),
                   None if prior is None else prior.abs())
    r = ratio("gemm_small_m" if small else "gemm_tile", (M, N, K), out.t, ref, 2 * (2 * K + 3) * U * mag, what)
    out.check(what)
    return small, r


@pytest.mark.parametrize("N,K", [(1000, 512), (512, 1000), (10, 64), (16, 70), (33, 65)])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 32])
def test_gemm_small_m(C, M, N, K):
    """Second accumulator used / unused / partly used (M = 17), waves with an empty or a
    partial K range (K = 64, 65, 70, 1000), N not a multiple of 16."""
    assert run_gemm(C, M, N, K)[0]
    assert run_gemm(C, M, N, K, bias=False, b_kn=True)[0]


@pytest.mark.parametrize("kw", [dict(a_bf16=True), dict(b_bf16=True), dict(a_bf16=True, b_bf16=True),
                                dict(alpha=0.37), dict(accum=True), dict(accum=True, alpha=0.37, bias=False),
                                dict(a_layout="km"), dict(a_layout="km", b_kn=True, accum=True)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("M,N,K", [(17, 1000, 512), (5, 33, 65)])
def test_gemm_small_m_variants(C, M, N, K, kw):
    assert run_gemm(C, M, N, K, **kw)[0]


@pytest.mark.parametrize("N,K", [(1000, 64), (33, 70)])
@pytest.mark.parametrize("accum", [False, True])
def test_gemm_small_m_ones_row(C, N, K, accum):
    """The bias-gradient call: a ones row read with sam = 0, B = dlogits [K,N]."""
    assert run_gemm(C, 1, N, K, a_layout="ones", b_kn=True, bias=False, accum=accum)[0]


@pytest.mark.parametrize("M,N,K", [(33, 1000, 512), (64, 512, 1000), (1000, 512, 5), (1000, 512, 32),
                                   (17, 33, 63), (1, 1000, 32)])
def test_gemm_tile(C, M, N, K):
    assert not run_gemm(C, M, N, K)[0]
    assert not run_gemm(C, M, N, K, bias=False, accum=True, b_kn=True)[0]
    assert not run_gemm(C, M, N, K, a_layout="km", alpha=0.37, accum=True)[0]
    if K <= 32:
        assert not run_gemm(C, M, N, K, a_bf16=True, b_bf16=True, b_kn=True)[0]


@pytest.mark.parametrize("B", [1, 5, 33, 64])
def test_linear_head_per_element(C, B):
    """linear_head end to end: out, dx, dW, db per element.  B = 33 moves the forward and dx
    onto the tile kernel; at B = 64 the sam = 0 bias-gradient call lands on the small-M kernel."""
    from ddp_amd.ops.resnet_fn import linear_head

    K, N = 512, 1000
    x = rnd(B, K, seed=51, dtype=F32).requires_grad_(True)
    w = rnd(N, K, scale=0.05, seed=52, dtype=F32).requires_grad_(True)
    b = rnd(N, scale=0.1, seed=53, dtype=F32).requires_grad_(True)
    out = linear_head(x, w, b)
    dl = rnd(B, N, seed=54, dtype=F32)
    out.backward(dl)
    torch.cuda.synchronize()
    xd, wd, bd, dd = f64(x), f64(w), f64(b), f64(dl)
    what = f"linear_head B={B}"

    def bound(Kc, mag):
        return 2 * (2 * Kc + 3) * U * mag

    ratio("head_out", (B, N, K), out, xd @ wd.t() + bd, bound(K, xd.abs() @ wd.abs().t() + bd.abs()), what)
    ratio("head_dx", (B, N, K), x.grad, dd @ wd, bound(N, dd.abs() @ wd.abs()), what)
    ratio("head_dw", (B, N, K), w.grad, dd.t() @ xd, bound(B, dd.abs().t() @ xd.abs()), what)
    ratio("head_db", (B, N, K), b.grad, dd.sum(0), bound(B, dd.abs().sum(0)), what)


# --------------------------------------------------------------------------- cross-entropy
def xent_inputs(B, NC):
    g = torch.Generator().manual_seed(61 + B + NC)
    lg = torch.randn(B, NC, generator=g) * 3
    for i in range(B):
        kind = i % 4
        if kind == 0:
            lg[i] += 1e4                                   # large offset
        elif kind == 1:
            lg[i] = 2.5                                    # all logits equal
        elif kind == 2:
            lo, hi = lg[i].min(), lg[i].max()
            lg[i] = (lg[i] - lo) / (hi - lo) * 60.0 - 20   # a spread of 60
    lab = torch.randint(0, NC, (B,), generator=g)
    forced = [NC - 1, min(64, NC - 1), min(63, NC - 1), 0]  # lane / step boundaries and the last class
    for i, v in enumerate(forced[:B]):
        lab[i] = v
    return lg.to(dev), lab.to(dev)


def run_xent(C, B, NC, family):
    lg, lab = xent_inputs(B, NC)
    gscale = torch.tensor(1.0 / B, dtype=F32).item()  # what the kernel receives: 1 / B in float32
    dl, loss = Guarded((B, NC), F32), Guarded((1,), F32)
    C.xent(lg, 1, None, lab, None, dl.t, loss.t, None, gscale, 0.0)
    torch.cuda.synchronize()
    what = f"xent {(B, NC)}"
    rows, p = R.xent_rows64(lg, lab)
    loss_ref, dl_ref = R.xent64(lg, lab, gscale)
    x = f64(lg)
    D = (x - x.max(1, keepdim=True).values).abs().max(1).values
    ratio(family + "_dlogits", (B, NC), dl.t, dl_ref, gscale * (p * (2 * D[:, None] + 64) * U + 2 * U), what)
    lb = ((D + 64) * U * rows.abs().clamp(min=1.0)).mean()
    ratio(family + "_loss", (B, NC), loss.t, loss_ref.reshape(1), lb.reshape(1), what)
    dl.check(what)
    loss.check(what)
    loss2 = Guarded((1,), F32)
    C.xent(lg, 1, None, lab, None, dl.t, loss2.t, None, gscale, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(bits(loss.t), bits(loss2.t)), f"{what}: the loss is not run-to-run identical"


@pytest.mark.parametrize("B,NC", [(1, 65), (4, 1000), (5, 1000), (7, 1024), (9, 127), (130, 1000)])
def test_xent_wave_rows(C, B, NC):
    """One wave per row (G = 1, no bias, int64 labels, more than 64 classes)."""
    run_xent(C, B, NC, "xent_wave")


def test_xent_block_kernel(C):
    """The same assertions through the one-block kernel (10 classes)."""
    run_xent(C, 7, 10, "xent_block")
