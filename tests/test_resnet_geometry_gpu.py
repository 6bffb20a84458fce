"""ResNet conv kernels at odd, non-square and off-224 geometries, per element, on MI355X.

`train_ddp.py --model resnet18 --image_size N` reaches any geometry (100 -> 50, 25, 13, 7, 4;
72 -> 36, 18, 9, 5, 3), the rest of the suite only the ImageNet-224 widths and powers of two.
Every kernel is compared with a float64 CPU reference of the same operation on the same
bf16 inputs, element by element, against an a-priori rounding bound (nothing calibrated on
the kernels).  The kernels multiply bf16 operands exactly in fp32, accumulate in fp32 in
some order and round a bf16 output once; with u = 2**-24, n the accumulated terms of one
output element and A the same convolution of the operands' absolute values:

    bf16 outputs (y, dx):       |out - ref| <= 2**-8 |ref| + 2 n u A + 1e-30
    fp32 outputs (dw):          |out - ref| <= 2 n u A + 1e-30
    BatchNorm statistics slab:  |sum - S|   <= 2 P u S_abs   (S from the stored bf16 y, fp64)

The factor 2 covers the split-K / slab re-summation.  Accumulate mode adds the prior value as
one more term of the same sum (n + 1 terms, A + |prior|) - the formula applied to what the
kernel computes, not a wider one.  profiles/resnet_geometry/README.md records the largest
observed error / bound per kernel family (run with -s to print them).

Every output, the split-K workspace and every slab is carved out of a larger buffer with
sentinel bands on both sides (nothing outside is written) and pre-filled with NaN (every
element is written); masked data-gradient elements are exactly 0.
"""
import pytest
import torch
import torch.nn.functional as F

from elementwise import BF, Guarded, U, f64, nchw, nhwc, report_ratio, rnd

pytestmark = pytest.mark.gpu
dev = "cuda"


def ratio_bf16(out, ref, A, n, what):
    """max |out - ref| / bound of a bf16 output; asserts every element written and in bound."""
    o = f64(out)
    assert bool(torch.isfinite(o).all()), f"{what}: unwritten / non-finite elements"
    bound = 2.0 ** -8 * ref.abs() + 2 * n * U * A + 1e-30
    r = ((o - ref).abs() / bound).max().item()
    assert r <= 1.0, f"{what}: error / bound = {r:.3f}"
    return r


def ratio_f32(out, ref, A, n, what):
    o = f64(out)
    assert bool(torch.isfinite(o).all()), f"{what}: unwritten / non-finite elements"
    bound = 2 * n * U * A + 1e-30
    r = ((o - ref).abs() / bound).max().item()
    assert r <= 1.0, f"{what}: error / bound = {r:.3f}"
    return r


def ratio_stats(stats, y, what):
    """Stats slab [rows][2][C] summed over rows (fp64) vs the stored bf16 y."""
    s = f64(stats)
    assert bool(torch.isfinite(s).all()), f"{what}: unwritten stats rows"
    s = s.sum(0)
    yd = f64(y).reshape(-1, y.shape[-1])
    P = yd.shape[0]
    b0 = 2 * P * U * yd.abs().sum(0) + 1e-30
    b1 = 2 * P * U * (yd * yd).sum(0) + 1e-30
    r = max(((s[0] - yd.sum(0)).abs() / b0).max().item(), ((s[1] - (yd * yd).sum(0)).abs() / b1).max().item())
    assert r <= 1.0, f"{what}: stats error / bound = {r:.3f}"
    return r


def report(family, shape, r):
    report_ratio(r, family, shape, tag="GEOM_RATIO")


class Conv:
    """Inputs and float64 references of one convolution (computed once per shape)."""

    def __init__(self, N, H, W, Cin, Cout, K, s, p, seed=0):
        self.geo = (N, H, W, Cin, Cout, K, s, p)
        self.OH, self.OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        self.x = rnd(N, H, W, Cin, relu=True, seed=seed + 1)
        self.w = rnd(Cout, K, K, Cin, scale=0.05, seed=seed + 2)
        self.dy = rnd(N, self.OH, self.OW, Cout, scale=0.5, seed=seed + 3)
        xd, wd, dyd = nchw(self.x), nchw(self.w), nchw(self.dy)
        kw = dict(stride=s, padding=p)
        self.y_ref = nhwc(F.conv2d(xd, wd, **kw))
        self.y_abs = nhwc(F.conv2d(xd.abs(), wd.abs(), **kw))
        self.dx_ref = nhwc(torch.nn.grad.conv2d_input(xd.shape, wd, dyd, **kw))
        self.dx_abs = nhwc(torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dyd.abs(), **kw))
        self.dw_ref = nhwc(torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, **kw)).reshape(-1)
        self.dw_abs = nhwc(torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), **kw)).reshape(-1)
        self.xpos = f64(self.x) > 0
        self.P = N * self.OH * self.OW
        self.row = Cout * K * K * Cin


_CACHE = {}


def conv_case(*geo):
    if geo not in _CACHE:
        _CACHE[geo] = Conv(*geo)
    return _CACHE[geo]


def run_fwd(C, cv, bp, bc, splits, halo, want_halo=None):
    N, H, W, Cin, Cout, K, s, p = cv.geo
    y = Guarded((N, cv.OH, cv.OW, Cout), BF)
    pbp, pbc, sp, rows, _, hl = C.conv_gemm_plan(cv.x, y.t, K, K, s, p, False, bp, bc, splits, -1, halo)
    if want_halo is not None:
        assert hl == want_halo, (cv.geo, hl)
    if splits > 0:
        assert sp == splits
    stats = Guarded((rows, 2, Cout), torch.float32)
    part = Guarded((sp * y.t.numel(),), torch.float32) if sp > 1 else None
    C.conv_gemm_fwd(cv.x, cv.w, None, y.t, K, K, s, p, False, stats.t, part.t if part else None, bp, bc,
                    splits, halo)
    torch.cuda.synchronize()
    what = f"fwd {cv.geo} plan bp={pbp} bc={pbc} splits={sp} halo={hl}"
    r = ratio_bf16(y.t, cv.y_ref, cv.y_abs, K * K * Cin, what)
    rs = ratio_stats(stats.t, y.t, what)
    for g_ in (y, stats, part):
        if g_ is not None:
            g_.check(what)
    return r, rs, hl


def run_dgrad(C, cv, bp, bc, splits, parity, halo, mask, want_halo=None):
    N, H, W, Cin, Cout, K, s, p = cv.geo
    dx = Guarded((N, H, W, Cin), BF)
    pbp, pbc, sp, _, par, hl = C.conv_gemm_plan(cv.x, cv.dy, K, K, s, p, True, bp, bc, splits, parity, halo)
    if want_halo is not None:
        assert hl == want_halo, (cv.geo, hl)
    assert par == (1 if (s == 2 and parity != 0) else 0)
    part = Guarded((sp * dx.t.numel(),), torch.float32) if sp > 1 else None
    C.conv_gemm_dgrad(cv.dy, cv.w, cv.x if mask else None, dx.t, K, K, s, p, part.t if part else None, bp, bc,
                      splits, parity, halo)
    torch.cuda.synchronize()
    what = f"dgrad {cv.geo} plan bp={pbp} bc={pbc} splits={sp} parity={par} halo={hl} mask={mask}"
    ref, A = cv.dx_ref, cv.dx_abs
    if mask:
        ref = torch.where(cv.xpos, ref, torch.zeros_like(ref))
        got = f64(dx.t)
        assert bool((got[~cv.xpos] == 0).all()), f"{what}: masked elements must be exactly 0"
    r = ratio_bf16(dx.t, ref, A, K * K * Cout, what)
    for g_ in (dx, part):
        if g_ is not None:
            g_.check(what)
    return r, hl


def run_wgrad(C, cv, ppc, accum=False, ks=0):
    """Weight gradient with `ppc` pixels per chunk: slabs + grad_reduce when chunked, the
    gradient itself for one chunk; `accum` adds onto a random prior.  Returns error / bound."""
    N, H, W, Cin, Cout, K, s, p = cv.geo
    ch = C.conv_gemm_wgrad_chunks(cv.x, cv.dy, K, K, s, p, ppc)
    assert ch * ppc >= cv.P > (ch - 1) * ppc
    g = torch.Generator().manual_seed(77)
    prior = torch.randn(cv.row, generator=g).to(dev)
    dw = Guarded((cv.row,), torch.float32)
    if accum:
        dw.t.copy_(prior)
    slab = None
    if ch == 1:
        C.conv_gemm_wgrad(cv.dy, cv.x, dw.t, K, K, s, p, ppc, accum, ks)
    else:
        slab = Guarded((ch, cv.row), torch.float32)
        C.conv_gemm_wgrad(cv.dy, cv.x, slab.t, K, K, s, p, ppc, False, ks)
        C.grad_reduce([(slab.t, cv.row, 0, cv.row, ch, dw.t, 1.0, accum)])
    torch.cuda.synchronize()
    what = f"wgrad {cv.geo} ppc={ppc} chunks={ch} accum={accum} ks={ks}"
    if slab is not None:
        assert bool(torch.isfinite(slab.t).all()), f"{what}: unwritten slab elements"
        slab.check(what)
    dw.check(what)
    if accum:  # the prior is one more term of the sum
        pd = f64(prior)
        return ratio_f32(dw.t, pd + cv.dw_ref, cv.dw_abs + pd.abs(), cv.P + 1, what)
    return ratio_f32(dw.t, cv.dw_ref, cv.dw_abs, cv.P, what)


def ceil32(v):
    return -(-v // 32) * 32


# (N, H, W, Cin, Cout) -> is the tap-fused halo weight gradient eligible (224 % Wp == 0 with
# Wp = W rounded up to 8, and the stacked halos fit its LDS tile)
S1_SHAPES = {
    (2, 13, 13, 64, 64): True,    # odd; halo R = 9, partial group of 4; wgrad Wp = 16, one 13-row image per group
    (3, 5, 5, 64, 128): True,     # R > H; wgrad stacks 5 images per group with N = 3; P = 75
    (2, 10, 20, 64, 64): False,   # non-square; Wp = 24 does not divide the 224 slots
    (2, 20, 10, 64, 64): True,    # non-square the other way; wgrad groups of 14 + 6 rows
    (1, 25, 25, 128, 64): True,   # Wp = 32 padded columns, 4 channel chunks
    (1, 9, 50, 64, 64): True,     # Wp = 56, halo R = 2 with a last group of one row
    (1, 18, 18, 64, 64): False,   # Wp = 24: per-tap GEMM with P = 324
    (2, 6, 3, 64, 64): True,      # W = 3: Wp = 8, 4 stacked 6-row images (320 of 360 halo positions)
}
S1 = list(S1_SHAPES)


@pytest.mark.parametrize("N,H,W,Cin,Cout", S1)
def test_stride1_fwd_stats(C, N, H, W, Cin, Cout):
    """3x3 / s1 forward + BatchNorm statistics: the auto plan, the gathered GEMM and the LDS
    halo tile (generic width, partial last row group, R > H), each unsplit and split in 2."""
    cv = conv_case(N, H, W, Cin, Cout, 3, 1, 1)
    R128 = 128 // W
    assert (R128 + 2) * (W + 2) <= 232  # every shape here fits the halo tile: forcing must be honoured
    rmax, smax = 0.0, 0.0
    for bp, bc, splits, halo, want in ((0, 0, 0, -1, None), (0, 0, 1, 0, 0), (0, 0, 2, 0, 0),
                                       (0, 0, 1, 1, 1), (0, 0, 2, 1, 1), (64, 0, 1, 1, 1), (0, 0, 0, 1, 1)):
        r, rs, hl = run_fwd(C, cv, bp, bc, splits, halo, want)
        report("fwd_halo" if hl else "fwd_gemm", cv.geo, r)
        report("stats", cv.geo, rs)
        rmax, smax = max(rmax, r), max(smax, rs)
    if Cout % 128 == 0:  # the 128-channel halo tile
        r, rs, _ = run_fwd(C, cv, 0, 128, 1, 1, 1)
        report("fwd_halo", cv.geo, r)


@pytest.mark.parametrize("N,H,W,Cin,Cout", S1)
def test_stride1_dgrad(C, N, H, W, Cin, Cout):
    """3x3 / s1 data gradient, with and without the ReLU mask, under the same plans."""
    cv = conv_case(N, H, W, Cin, Cout, 3, 1, 1)
    for bp, bc, splits, halo, want in ((0, 0, 0, -1, None), (0, 0, 1, 0, 0), (0, 0, 2, 0, 0),
                                       (0, 0, 1, 1, 1), (0, 0, 2, 1, 1), (64, 0, 1, 1, 1), (0, 0, 0, 1, 1)):
        for mask in (False, True):
            r, hl = run_dgrad(C, cv, bp, bc, splits, -1, halo, mask, want)
            report("dgrad_halo" if hl else "dgrad_gemm", cv.geo, r)
    if Cin % 128 == 0:
        r, _ = run_dgrad(C, cv, 0, 128, 1, -1, 1, True, 1)
        report("dgrad_halo", cv.geo, r)


@pytest.mark.parametrize("N,H,W,Cin,Cout", S1)
def test_stride1_wgrad(C, N, H, W, Cin, Cout):
    """3x3 / s1 weight gradient: the planner's own chunking, one chunk written and one
    accumulated, and the tap-fused halo kernel (32 and 16 input channels per block) against
    the per-tap GEMM kernel - both per element against float64."""
    cv = conv_case(N, H, W, Cin, Cout, 3, 1, 1)
    elig = S1_SHAPES[(N, H, W, Cin, Cout)]
    a = (cv.x, cv.dy, 3, 3, 1, 1)
    one_gemm = ceil32(cv.P)
    try:
        # the default configuration: what the trainer runs
        ppc = C.conv_gemm_wgrad_ppc(*a)
        assert C.conv_gemm_wgrad_uses_halo(*a, ppc) == elig
        fam = "wgrad_halo" if elig else "wgrad_gemm"
        report(fam, cv.geo, run_wgrad(C, cv, ppc))
        one = cv.P if elig else one_gemm
        assert C.conv_gemm_wgrad_uses_halo(*a, one) == elig
        assert C.conv_gemm_wgrad_chunks(*a, one) == 1
        report(fam, cv.geo, run_wgrad(C, cv, one))
        report(fam, cv.geo, run_wgrad(C, cv, one, accum=True))
        # halo kernel wherever eligible, both block widths; smaller chunks (whole rows, whole
        # images when stacked) so that chunk boundaries fall inside the batch
        for cit in (32, 16):
            C.conv_gemm_wgrad_set_halo(2, 256, cit)
            assert C.conv_gemm_wgrad_uses_halo(*a, cv.P) == elig
            if not elig:
                continue
            q = H if H < 224 // ((W + 7) & ~7) else 1  # rows per chunk: whole images when stacked
            for rows in sorted({q, 3 * q, C.conv_gemm_wgrad_ppc(*a) // W}):
                assert C.conv_gemm_wgrad_uses_halo(*a, rows * W)
                report("wgrad_halo", cv.geo, run_wgrad(C, cv, rows * W))
            report("wgrad_halo", cv.geo, run_wgrad(C, cv, cv.P))
            report("wgrad_halo", cv.geo, run_wgrad(C, cv, cv.P, accum=True))
        # the per-tap GEMM kernel on the same shape (P % 32 != 0: a ragged last K-step)
        C.conv_gemm_wgrad_set_halo(0)
        assert not C.conv_gemm_wgrad_uses_halo(*a, one_gemm)
        for ks in (32, 64):
            report("wgrad_gemm", cv.geo, run_wgrad(C, cv, one_gemm, ks=ks))
        report("wgrad_gemm", cv.geo, run_wgrad(C, cv, one_gemm, accum=True))
        report("wgrad_gemm", cv.geo, run_wgrad(C, cv, 64, accum=True))
    finally:
        C.conv_gemm_wgrad_set_halo(1)


S2 = [(2, 13, 13, 64, 128), (3, 5, 7, 64, 128), (2, 9, 9, 128, 256), (1, 25, 25, 64, 128)]
K2 = [(3, 1), (1, 0)]


@pytest.mark.parametrize("K,p", K2)
@pytest.mark.parametrize("N,H,W,Cin,Cout", S2)
def test_stride2_fwd_stats(C, N, H, W, Cin, Cout, K, p):
    """Stride-2 3x3 / 1x1 forward + statistics from odd and non-square inputs."""
    cv = conv_case(N, H, W, Cin, Cout, K, 2, p)
    for bp, bc, splits in ((0, 0, 0), (0, 0, 1), (0, 0, 2), (128, 128, 1), (64, 64, 2)):
        r, rs, _ = run_fwd(C, cv, bp, bc, splits, -1, 0)
        report("fwd_gemm_s2", cv.geo, r)
        report("stats", cv.geo, rs)
    # the halo tile is stride-1 only: forcing it must be refused by the planner, not mis-run
    assert run_fwd(C, cv, 0, 0, 0, 1, 0)[2] == 0


@pytest.mark.parametrize("K,p", K2)
@pytest.mark.parametrize("N,H,W,Cin,Cout", S2)
def test_stride2_dgrad(C, N, H, W, Cin, Cout, K, p):
    """Stride-2 data gradient from an odd input: parity classes of unequal size (the smaller
    classes' surplus blocks return early), plain 9-tap GEMM, split K, ReLU mask."""
    cv = conv_case(N, H, W, Cin, Cout, K, 2, p)
    for parity in (-1, 0):
        for splits in (0, 2):
            for mask in (False, True):
                r, _ = run_dgrad(C, cv, 0, 0, splits, parity, -1, mask, 0)
                report("dgrad_parity" if parity else "dgrad_gemm_s2", cv.geo, r)
    r, _ = run_dgrad(C, cv, 64, 64, 1, -1, -1, True, 0)  # 64-pixel tiles: more blocks per class
    report("dgrad_parity", cv.geo, r)


@pytest.mark.parametrize("K,p", K2)
@pytest.mark.parametrize("N,H,W,Cin,Cout", S2)
def test_stride2_wgrad(C, N, H, W, Cin, Cout, K, p):
    cv = conv_case(N, H, W, Cin, Cout, K, 2, p)
    a = (cv.x, cv.dy, K, K, 2, p)
    ppc = C.conv_gemm_wgrad_ppc(*a)
    assert ppc % 32 == 0 and not C.conv_gemm_wgrad_uses_halo(*a, ppc)
    one = ceil32(cv.P)
    for args in ((ppc,), (one,), (one, True), (32, True), (64, False, 64)):
        report("wgrad_gemm_s2", cv.geo, run_wgrad(C, cv, *args))


@pytest.mark.parametrize("N,H,W", [(2, 45, 45), (1, 30, 50)])
def test_stem_odd_and_nonsquare(C, N, H, W):
    """7x7 / s2 / p3 stem (Cin = 4 via to_nhwc4) with an odd OH (23) and with OH != OW
    (15 x 25): forward with and without the statistics slab, and the weight gradient."""
    from ddp_amd.ops.resnet_fn import to_nhwc4

    g = torch.Generator().manual_seed(5)
    x4 = to_nhwc4(torch.randn(N, 3, H, W, generator=g).to(dev))
    w4 = F.pad(torch.randn(64, 7, 7, 3, generator=g) * 0.05, (0, 1)).to(BF).to(dev).contiguous()
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = rnd(N, OH, OW, 64, scale=0.5, seed=6)
    xd, wd, dyd = nchw(x4[..., :3]), nchw(w4[..., :3]), nchw(dy)
    kw = dict(stride=2, padding=3)
    y_ref, y_abs = nhwc(F.conv2d(xd, wd, **kw)), nhwc(F.conv2d(xd.abs(), wd.abs(), **kw))
    geo = (N, H, W, 4, 64, 7, 2, 3)
    ys = []
    for with_stats in (False, True):
        y = Guarded((N, OH, OW, 64), BF)
        rows = C.conv_gemm_plan(x4, y.t, 7, 7, 2, 3)[3]
        assert rows == -(-N * OH * OW // 128)
        stats = Guarded((rows, 2, 64), torch.float32) if with_stats else None
        C.conv_gemm_fwd(x4, w4, None, y.t, 7, 7, 2, 3, False, stats.t if stats else None)
        torch.cuda.synchronize()
        report("stem_fwd", geo, ratio_bf16(y.t, y_ref, y_abs, 147, f"stem fwd {geo} stats={with_stats}"))
        y.check("stem y")
        if stats:
            report("stats", geo, ratio_stats(stats.t, y.t, f"stem {geo}"))
            stats.check("stem stats")
        ys.append(y.t)
    assert torch.equal(ys[0], ys[1])
    # weight gradient [Cout][7][7][3] (the pad channel is dropped)
    dw_ref = nhwc(torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, **kw)).reshape(-1)
    dw_abs = nhwc(torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), **kw)).reshape(-1)
    row, P = 64 * 49 * 3, N * OH * OW
    a = (x4, dy, 7, 7, 2, 3)
    for ppc in (C.conv_gemm_wgrad_ppc(*a), 64, ceil32(P)):
        ch = C.conv_gemm_wgrad_chunks(*a, ppc)
        dw = Guarded((row,), torch.float32)
        if ch == 1:
            C.conv_gemm_wgrad(dy, x4, dw.t, 7, 7, 2, 3, ppc, False)
        else:
            slab = Guarded((ch, row), torch.float32)
            C.conv_gemm_wgrad(dy, x4, slab.t, 7, 7, 2, 3, ppc, False)
            C.grad_reduce([(slab.t, row, 0, row, ch, dw.t, 1.0, False)])
            torch.cuda.synchronize()
            assert bool(torch.isfinite(slab.t).all())
            slab.check("stem slab")
        torch.cuda.synchronize()
        report("stem_wgrad", geo, ratio_f32(dw.t, dw_ref, dw_abs, P, f"stem wgrad {geo} ppc={ppc}"))
        dw.check("stem dw")


@pytest.mark.parametrize("H,W", [(3, 3), (4, 4), (3, 4)])
def test_halo_wgrad_gate_small_images(C, H, W):
    """Images whose stacked halos exceed the halo weight gradient's LDS tile (3 x 3: 9 images x
    5 x 10 = 450 positions > 360; 4 x 4: 420) are refused by the planner - the per-tap GEMM
    runs instead (ResNet-18's last stage at image sizes 72 .. 128) and is right."""
    cv = conv_case(2, H, W, 64, 64, 3, 1, 1)
    a = (cv.x, cv.dy, 3, 3, 1, 1)
    try:
        C.conv_gemm_wgrad_set_halo(2, 256, 32)
        ppc = C.conv_gemm_wgrad_ppc(*a)
        assert ppc % 32 == 0
        for v in (ppc, cv.P, H * W, ceil32(cv.P)):
            assert not C.conv_gemm_wgrad_uses_halo(*a, v)
        report("wgrad_gemm", cv.geo, run_wgrad(C, cv, ppc))
        report("wgrad_gemm", cv.geo, run_wgrad(C, cv, ppc, accum=True))
    finally:
        C.conv_gemm_wgrad_set_halo(1)
    r, _, _ = run_fwd(C, cv, 0, 0, 1, 1, 1)
    report("fwd_halo", cv.geo, r)
    r, _ = run_dgrad(C, cv, 0, 0, 1, -1, 1, True, 1)
    report("dgrad_halo", cv.geo, r)
