"""ResNet-18 kernels (conv_gemm, BatchNorm, pooling, head) vs plain PyTorch fp32 on MI355X."""
import pytest
import torch
import torch.nn.functional as F

from elementwise import BF, rnd

pytestmark = pytest.mark.gpu
dev = "cuda"


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


CASES = [  # N, H, Cin, Cout, K, stride, pad
    (4, 14, 64, 64, 3, 1, 1),
    (2, 28, 64, 128, 3, 1, 1),     # halo-tile forward (W = 28, 4 rows per block)
    (1, 56, 128, 64, 3, 1, 1),     # halo-tile forward (W = 56, 2 rows), 4 channel chunks
    (4, 14, 64, 128, 3, 2, 1),
    (4, 14, 64, 128, 1, 2, 0),
    (2, 8, 256, 512, 3, 2, 1),
    (2, 7, 512, 512, 3, 1, 1),
]
PLANS = [(0, 0, 0), (64, 64, 1), (128, 128, 1), (64, 128, 3), (128, 64, 2), (0, 0, 2)]  # (bp, bc, splits); 0 = auto


@pytest.mark.parametrize("N,H,Cin,Cout,splits,bc,bp", [(4, 14, 64, 64, 1, 64, 0), (4, 14, 64, 64, 1, 64, 128),
                                                        (2, 28, 64, 128, 2, 128, 0), (2, 28, 64, 128, 1, 64, 64),
                                                        (1, 56, 128, 64, 2, 64, 0), (3, 56, 64, 64, 1, 0, 0),
                                                        (2, 7, 64, 128, 1, 0, 0)])
def test_halo_fwd_forced(C, N, H, Cin, Cout, splits, bc, bp):
    """The LDS halo-tile forward (conv_halo.hip), forced on: both pixel tiles, both channel
    tiles, with and without K splits, down to the 7-wide layer."""
    x = rnd(N, H, H, Cin, relu=True, seed=11)
    w = rnd(Cout, 3, 3, Cin, scale=0.05, seed=12)
    y = torch.empty(N, H, H, Cout, dtype=BF, device=dev)
    pbp, _, sp, rows, _, halo = C.conv_gemm_plan(x, y, 3, 3, 1, 1, False, bp, bc, splits, -1, 1)
    assert halo == 1 and sp == splits and (bp == 0 or pbp == bp)
    stats = torch.empty(rows, 2, Cout, device=dev)
    part = torch.empty(sp * y.numel(), device=dev) if sp > 1 else None
    C.conv_gemm_fwd(x, w, None, y, 3, 3, 1, 1, False, stats, part, bp, bc, splits, 1)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    assert relerr(y, ref) < 1e-2
    st = stats.sum(0)
    yb = y.float()
    assert relerr(st[0], yb.sum((0, 1, 2))) < 1e-4 and relerr(st[1], (yb * yb).sum((0, 1, 2))) < 1e-4
    # the halo data gradient (dY halo, flipped taps, transposed weight reads), same tiles
    if Cin % 64 == 0 and (bc == 0 or Cin % bc == 0):
        dy = rnd(N, H, H, Cout, scale=0.5, seed=13)
        rdx = torch.nn.grad.conv2d_input(x.shape[:1] + (Cin, H, H), w.float().permute(0, 3, 1, 2),
                                         dy.float().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
        for mask in (None, x):
            dx = torch.full_like(x, 3.0)
            _, _, sd, _, _, hd = C.conv_gemm_plan(x, dy, 3, 3, 1, 1, True, bp, bc, splits, -1, 1)
            assert hd == 1
            partd = torch.empty(sd * x.numel(), device=dev) if sd > 1 else None
            C.conv_gemm_dgrad(dy, w, mask, dx, 3, 3, 1, 1, partd, bp, bc, splits, -1, 1)
            want = rdx if mask is None else torch.where(x.float() > 0, rdx, torch.zeros_like(rdx))
            assert relerr(dx, want) < 1e-2, mask is not None


def _plan_ok(bp, bc, C):
    return bc == 0 or C % bc == 0


@pytest.mark.parametrize("N,H,Cin,Cout,K,s,p", CASES)
@pytest.mark.parametrize("bp,bc,splits", PLANS)
def test_conv_gemm_fwd_dgrad(C, N, H, Cin, Cout, K, s, p, bp, bc, splits):
    """Forward (+ BN statistics) and data gradient (+ ReLU mask) of every launch plan:
    pixel tile, channel tile, split-K (fp32 partials + fixed-order splitk_reduce)."""
    OH = (H + 2 * p - K) // s + 1
    x = rnd(N, H, H, Cin, relu=True, seed=1)
    w = rnd(Cout, K, K, Cin, scale=0.05, seed=2)
    xr = x.float().permute(0, 3, 1, 2)
    wr = w.float().permute(0, 3, 1, 2)
    if _plan_ok(bp, bc, Cout):
        y = torch.empty(N, OH, OH, Cout, dtype=BF, device=dev)
        _, _, sp, rows, _, _ = C.conv_gemm_plan(x, y, K, K, s, p, False, bp, bc, splits)
        stats = torch.empty(rows, 2, Cout, device=dev)
        part = torch.empty(sp * y.numel(), device=dev) if sp > 1 else None
        C.conv_gemm_fwd(x, w, None, y, K, K, s, p, False, stats, part, bp, bc, splits)
        ref = F.conv2d(xr, wr, stride=s, padding=p).permute(0, 2, 3, 1)
        assert relerr(y, ref) < 1e-2
        yb = y.float()
        st = stats.sum(0)
        assert relerr(st[0], yb.sum((0, 1, 2))) < 1e-4
        assert relerr(st[1], (yb * yb).sum((0, 1, 2))) < 1e-4
    if _plan_ok(bp, bc, Cin):
        dy = rnd(N, OH, OH, Cout, scale=0.5, seed=3)
        rdx = torch.nn.grad.conv2d_input(xr.shape, wr, dy.float().permute(0, 3, 1, 2), stride=s,
                                         padding=p).permute(0, 2, 3, 1)
        # stride 2: the parity-class decomposition (auto) and the plain 9-tap GEMM
        for par in ((-1, 0) if s == 2 else (-1,)):
            for mask in (None, x):
                dx = torch.full_like(x, 3.0)  # every element must be written (zeros included)
                _, _, sp, _, used, _ = C.conv_gemm_plan(x, dy, K, K, s, p, True, bp, bc, splits, par)
                assert used == (1 if (s == 2 and par != 0) else 0)
                part = torch.empty(sp * x.numel(), device=dev) if sp > 1 else None
                C.conv_gemm_dgrad(dy, w, mask, dx, K, K, s, p, part, bp, bc, splits, par)
                want = rdx if mask is None else torch.where(x.float() > 0, rdx, torch.zeros_like(rdx))
                assert relerr(dx, want) < 1e-2, (par, mask is not None)


@pytest.mark.parametrize("N,H,Cin,Cout,K,s,p", CASES)
def test_conv_gemm_wgrad(C, N, H, Cin, Cout, K, s, p):
    """Weight gradient: split over pixel chunks (slabs + fixed-order reduce, accumulate
    mode) and one chunk written straight into the gradient (overwrite / accumulate)."""
    OH = (H + 2 * p - K) // s + 1
    x = rnd(N, H, H, Cin, relu=True, seed=1)
    dy = rnd(N, OH, OH, Cout, scale=0.5, seed=3)
    rdw = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (Cout, Cin, K, K),
                                      dy.float().permute(0, 3, 1, 2), stride=s,
                                      padding=p).permute(0, 2, 3, 1)
    P = N * OH * OH
    row = Cout * K * K * Cin
    ppc = 64
    ch = C.conv_gemm_wgrad_chunks(x, dy, K, K, s, p, ppc)
    slab = torch.empty(ch, row, device=dev)
    C.conv_gemm_wgrad(dy, x, slab, K, K, s, p, ppc, False)
    prior = torch.randn(row, device=dev)
    dw = prior.clone()
    C.grad_reduce([(slab, row, 0, row, ch, dw, 1.0, True)])
    assert relerr((dw - prior).view(Cout, K, K, Cin), rdw) < 2e-3
    one = -(-P // 32) * 32
    assert C.conv_gemm_wgrad_chunks(x, dy, K, K, s, p, one) == 1
    for ks in (32, 64):  # pixels staged per barrier
        d1 = torch.full((row,), 7.0, device=dev)
        C.conv_gemm_wgrad(dy, x, d1, K, K, s, p, one, False, ks)
        assert relerr(d1.view(Cout, K, K, Cin), rdw) < 2e-3, ks
    d2 = prior.clone()
    C.conv_gemm_wgrad(dy, x, d2, K, K, s, p, one, True)
    assert relerr((d2 - prior).view(Cout, K, K, Cin), rdw) < 2e-3


@pytest.mark.parametrize("N,H,Cin,Cout,rpc", [
    (2, 56, 64, 64, 4), (2, 56, 64, 64, 12),      # W = 56: 4-row groups, chunks inside an image
    (3, 28, 128, 64, 8), (3, 28, 64, 128, 24),    # W = 28 (Wp 32, 7-row groups), chunks across images
    (2, 14, 256, 64, 16),                         # W = 14: padded columns, chunks across images
    (4, 7, 64, 512, 14), (8, 7, 64, 64, 21),      # W = 7: images stacked 4 per group (2 / 3 per chunk)
])
@pytest.mark.parametrize("cit", [32, 16])
def test_conv_halo_wgrad(C, N, H, Cin, Cout, rpc, cit):
    """Tap-fused stride-1 3x3 weight gradient (conv_halo.hip): whole-row chunks (row groups
    split at image boundaries), slabs + fixed-order reduce, a single chunk written /
    accumulated directly, and the planner's own chunking - against fp32 PyTorch and the
    per-tap GEMM kernel."""
    x = rnd(N, H, H, Cin, relu=True, seed=11)
    dy = rnd(N, H, H, Cout, scale=0.5, seed=13)
    rdw = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (Cout, Cin, 3, 3),
                                      dy.float().permute(0, 3, 1, 2), stride=1,
                                      padding=1).permute(0, 2, 3, 1)
    row = Cout * 9 * Cin
    C.conv_gemm_wgrad_set_halo(2, 256, cit)  # the halo kernel, cit input channels per block
    try:
        for ppc in (rpc * H, C.conv_gemm_wgrad_ppc(x, dy, 3, 3, 1, 1)):
            assert ppc % H == 0
            ch = C.conv_gemm_wgrad_chunks(x, dy, 3, 3, 1, 1, ppc)
            slab = torch.full((ch, row), float("nan"), device=dev)  # every slab element is written
            C.conv_gemm_wgrad(dy, x, slab, 3, 3, 1, 1, ppc, False)
            dw = torch.zeros(row, device=dev)
            C.grad_reduce([(slab, row, 0, row, ch, dw, 1.0, False)])
            assert relerr(dw.view(Cout, 3, 3, Cin), rdw) < 2e-3, ppc
        P = N * H * H  # one chunk: overwrite, then accumulate
        d1 = torch.full((row,), 7.0, device=dev)
        C.conv_gemm_wgrad(dy, x, d1, 3, 3, 1, 1, P, False)
        assert relerr(d1.view(Cout, 3, 3, Cin), rdw) < 2e-3
        prior = torch.randn(row, device=dev)
        d2 = prior.clone()
        C.conv_gemm_wgrad(dy, x, d2, 3, 3, 1, 1, P, True)
        assert relerr((d2 - prior).view(Cout, 3, 3, Cin), rdw) < 2e-3
        if P % 32 == 0:
            C.conv_gemm_wgrad_set_halo(0)  # the per-tap GEMM kernel on the same chunking
            d3 = torch.full((row,), 7.0, device=dev)
            C.conv_gemm_wgrad(dy, x, d3, 3, 3, 1, 1, P, False)
            assert relerr(d1, d3) < 1e-4
    finally:
        C.conv_gemm_wgrad_set_halo(1)


@pytest.mark.parametrize("N,H", [(2, 32), (1, 224)])  # 224: the constant-geometry stem kernels (StemGeo<1>)
def test_stem_conv_7x7_s2(N, H):
    from ddp_amd import native
    from ddp_amd.ops.resnet_fn import to_nhwc4

    C = native.require()
    img = torch.randn(N, 3, H, H, device=dev)
    x4 = to_nhwc4(img)
    w3 = torch.randn(64, 7, 7, 3) * 0.05
    w4 = F.pad(w3, (0, 1)).to(BF).to(dev).contiguous()
    OH = (H + 6 - 7) // 2 + 1
    y = torch.empty(N, OH, OH, 64, dtype=BF, device=dev)
    C.conv_gemm_fwd(x4, w4, None, y, 7, 7, 2, 3, False, None)
    ref = F.conv2d(x4[..., :3].float().permute(0, 3, 1, 2), w4[..., :3].float().permute(0, 3, 1, 2),
                   stride=2, padding=3).permute(0, 2, 3, 1)
    assert relerr(y, ref) < 1e-2
    # with the BatchNorm statistics slab (per-block sum / sum of squares of the stored bf16 y)
    rows = C.conv_gemm_plan(x4, y, 7, 7, 2, 3)[3]
    stats = torch.empty(rows, 2, 64, device=dev)
    y2 = torch.empty_like(y)
    C.conv_gemm_fwd(x4, w4, None, y2, 7, 7, 2, 3, False, stats)
    assert torch.equal(y2, y)
    yf = y.float().view(-1, 64)
    assert relerr(stats[:, 0].sum(0), yf.sum(0)) < 1e-4
    assert relerr(stats[:, 1].sum(0), (yf * yf).sum(0)) < 1e-4
    dy = rnd(N, OH, OH, 64, seed=5)
    rdw = torch.nn.grad.conv2d_weight(x4[..., :3].float().permute(0, 3, 1, 2), (64, 3, 7, 7),
                                      dy.float().permute(0, 3, 1, 2), stride=2, padding=3)
    ppc = 64
    ch = C.conv_gemm_wgrad_chunks(x4, dy, 7, 7, 2, 3, ppc)
    slab = torch.empty(ch, 64 * 49 * 3, device=dev)
    C.conv_gemm_wgrad(dy, x4, slab, 7, 7, 2, 3, ppc, False)  # [Cout][T][3]: pad channel dropped
    dw = torch.empty(64 * 49 * 3, device=dev)
    C.grad_reduce([(slab, 64 * 49 * 3, 0, 64 * 49 * 3, ch, dw, 1.0)])
    assert relerr(dw.view(64, 7, 7, 3), rdw.permute(0, 2, 3, 1)) < 2e-3


@pytest.mark.parametrize("P_img,Cc", [(8, 64), (56, 64), (7, 512), (14, 256)])
def test_batchnorm_fwd_bwd_matches_torch(C, P_img, Cc):
    N, H = 4, P_img
    x = rnd(N, H, H, Cc, seed=6)
    res = rnd(N, H, H, Cc, seed=7)
    gamma = (torch.rand(Cc) + 0.5).to(dev)
    beta = (torch.randn(Cc) * 0.1).to(dev)
    P = N * H * H
    xf = x.float()
    # stats slab of 37 per-block partials (uneven split of the pixels)
    cuts = torch.linspace(0, P, 38).long().tolist()
    xs = xf.view(P, Cc)
    slab = torch.stack([torch.stack([xs[a:b].sum(0), (xs[a:b] * xs[a:b]).sum(0)])
                        for a, b in zip(cuts[:-1], cuts[1:])]).contiguous()
    rows = slab.shape[0]
    rm, rv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
    nbt = torch.zeros((), dtype=torch.long, device=dev)
    mean, invstd = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
    ws = torch.empty(C.bn_finalize_groups(rows), 2, Cc, device=dev)
    C.bn_finalize(slab, rows, Cc, float(P), 1e-5, 0.1, rm, rv, mean, invstd, nbt, ws)
    assert nbt.item() == 1
    out = torch.empty_like(x)
    C.bn_apply(x, mean, invstd, gamma, beta, res, True, out)
    # torch reference (fp32, NCHW)
    bn = torch.nn.BatchNorm2d(Cc).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xr = xf.permute(0, 3, 1, 2).clone().requires_grad_(True)
    rr = res.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = torch.relu(bn(xr) + rr)
    assert relerr(out, ref.permute(0, 2, 3, 1)) < 1e-2
    assert relerr(rm, bn.running_mean) < 1e-5 and relerr(rv, bn.running_var) < 1e-5
    dout = rnd(N, H, H, Cc, seed=8)
    ref.backward(dout.float().permute(0, 3, 1, 2))
    ws2 = torch.empty(C.bn_bwd_rows(P, Cc), 2, Cc, device=dev)
    sums = torch.empty(2 * Cc, device=dev)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x)
    dg0, db0 = torch.randn(Cc, device=dev), torch.randn(Cc, device=dev)
    dg, db = dg0.clone(), db0.clone()
    C.bn_bwd(dout, out, x, mean, invstd, gamma, float(P), ws2, sums, dg, db, True, dx, dres)
    assert relerr(dx, xr.grad.permute(0, 2, 3, 1)) < 2e-2
    assert relerr(dres, rr.grad.permute(0, 2, 3, 1)) < 1e-2
    assert relerr(sums[Cc:], bn.weight.grad) < 1e-3 and relerr(sums[:Cc], bn.bias.grad) < 1e-3
    assert relerr(dg - dg0, bn.weight.grad) < 1e-3 and relerr(db - db0, bn.bias.grad) < 1e-3
    # fixed-order reductions: a second run is bitwise identical
    sums2 = torch.empty_like(sums)
    C.bn_bwd(dout, out, x, mean, invstd, gamma, float(P), ws2, sums2, None, None, False, dx, None)
    assert torch.equal(sums, sums2)


@pytest.mark.parametrize("N,H,Cin,Cout,K,s,p", [
    (32, 56, 64, 64, 3, 1, 1),     # halo forward, 56 groups of rows
    (4, 14, 64, 128, 3, 2, 1),     # conv_gemm forward, two column blocks
    (2, 7, 512, 512, 3, 1, 1),     # split K -> splitk_reduce writes the stats (C = 512)
    (4, 14, 64, 128, 1, 2, 0),     # 1x1 downsample
    (2, 64, 4, 64, 7, 2, 3),       # stem (Cin 4): 128-pixel tiles, > 32 stats rows
])
def test_conv_stats_finalize_matches_torch(C, N, H, Cin, Cout, K, s, p):
    """The stats slab of every stats-producing forward plan (halo forward, conv_gemm with
    two column blocks, split K through splitk_reduce, 1x1 downsample, stem) finalised by
    bn_finalize: mean / invstd against torch's batch statistics of the same bf16 output,
    running stats with torch's momentum / unbiased-variance semantics, num_batches_tracked
    once per call, and a second call bitwise identical (self-resetting tickets)."""
    OH = (H + 2 * p - K) // s + 1
    x = rnd(N, H, H, Cin, relu=True, seed=21)
    if Cin == 4:
        x[..., 3] = 0
    w = rnd(Cout, K, K, Cin, scale=0.05, seed=22)
    y = torch.empty(N, OH, OH, Cout, dtype=BF, device=dev)
    _, _, sp, rows, _, _ = C.conv_gemm_plan(x, y, K, K, s, p)
    P = N * OH * OH
    part = torch.empty(sp * P * Cout, device=dev) if sp > 1 else None
    st = torch.empty(rows, 2, Cout, device=dev)
    C.conv_gemm_fwd(x, w, None, y, K, K, s, p, False, st, part)
    rm_init, rv_init = torch.rand(Cout, device=dev), torch.rand(Cout, device=dev) + 0.5
    yf = y.float().view(-1, Cout)
    outs = []
    for _ in range(2):
        rm, rv = rm_init.clone(), rv_init.clone()
        m, i = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
        nbt = torch.zeros((), dtype=torch.long, device=dev)
        ws = torch.full((C.bn_finalize_groups(rows), 2, Cout), float("nan"), device=dev)
        C.bn_finalize(st, rows, Cout, float(P), 1e-5, 0.1, rm, rv, m, i, nbt, ws)
        torch.cuda.synchronize()
        assert nbt.item() == 1
        assert relerr(m, yf.mean(0)) < 1e-4 and relerr(i, torch.rsqrt(yf.var(0, unbiased=False) + 1e-5)) < 1e-3
        assert relerr(rm, 0.9 * rm_init + 0.1 * yf.mean(0)) < 1e-4
        assert relerr(rv, 0.9 * rv_init + 0.1 * yf.var(0, unbiased=True)) < 1e-3
        outs.append((m, i, rm, rv))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rows,Cc", [(10, 64), (64, 128), (100, 512), (3136, 64), (5000, 64)])
def test_bn_finalize_row_counts(C, rows, Cc):
    """bn_finalize over 1 block per strip (<= 64 rows: no ticket), two levels (the ResNet-18
    stem's 3136 rows: 49 blocks) and more than 64 x 64 rows (128 rows per block, two load
    batches): mean / invstd / running stats against an fp64 reference, num_batches_tracked
    once, and bitwise reproducible."""
    g = torch.Generator().manual_seed(71)
    slab = (torch.randn(rows, 2, Cc, generator=g) * torch.tensor([1.0, 0.0])[None, :, None]).to(dev)
    slab[:, 1] = (torch.rand(rows, Cc, generator=g) * 4 + 1).to(dev)  # positive sums of squares
    count = float(rows * 64)
    res = []
    for _ in range(2):
        rm, rv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
        nbt = torch.zeros((), dtype=torch.long, device=dev)
        mean, invstd = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
        ws = torch.full((C.bn_finalize_groups(rows), 2, Cc), float("nan"), device=dev)
        C.bn_finalize(slab, rows, Cc, count, 1e-5, 0.1, rm, rv, mean, invstd, nbt, ws)
        torch.cuda.synchronize()
        assert nbt.item() == 1
        res.append((mean, invstd, rm, rv))
    sd = slab.double().sum(0).cpu()
    m_ref = sd[0] / count
    v_ref = (sd[1] / count - m_ref * m_ref).clamp_min(0)
    assert relerr(res[0][0], m_ref) < 1e-5
    assert relerr(res[0][1], torch.rsqrt(v_ref + 1e-5)) < 1e-5
    assert relerr(res[0][3], 0.9 + 0.1 * v_ref * count / (count - 1)) < 1e-5
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,H,Cc", [(32, 56, 64), (8, 14, 256), (4, 7, 512), (2, 5, 64)])
def test_bn_bwd_mask_from_input_bitwise(C, N, H, Cc):
    """BatchNorm + ReLU backward with the mask recomputed from the BN input (mask_beta:
    bf16(y * sc + sh) > 0 through bn_apply's own affine) == the backward that reads the
    output bn_apply stored: dx, sums, dgamma / dbeta bit for bit - including values that
    land exactly on / next to zero (a channel with beta = 0 and y == mean)."""
    P = N * H * H
    y = rnd(N, H, H, Cc, seed=41)
    y[..., 0] = 0  # channel 0: y == mean == 0 and beta 0 -> bn output exactly 0
    dout = rnd(N, H, H, Cc, seed=42)
    mean = torch.randn(Cc, device=dev) * 0.1
    mean[0] = 0
    invstd = torch.rand(Cc, device=dev) + 0.5
    gamma = torch.rand(Cc, device=dev) + 0.5
    beta = torch.randn(Cc, device=dev) * 0.3
    beta[0] = 0
    out = torch.empty_like(y)
    C.bn_apply(y, mean, invstd, gamma, beta, None, True, out)
    assert (out[..., 0] == 0).all() and (out > 0).any() and (out == 0).any()
    res = []
    for mode in ("out", "y"):
        ws = torch.empty(C.bn_bwd_rows(P, Cc), 2, Cc, device=dev)
        sums = torch.empty(2 * Cc, device=dev)
        dg, db = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
        dx = torch.empty_like(y)
        if mode == "out":
            C.bn_bwd(dout, out, y, mean, invstd, gamma, float(P), ws, sums, dg, db, False, dx, None)
        else:
            C.bn_bwd(dout, None, y, mean, invstd, gamma, float(P), ws, sums, dg, db, False, dx, None,
                     None, beta)
        torch.cuda.synchronize()
        res.append((dx, sums, dg, db))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("H,W", [(56, 56), (8, 11)])
def test_maxpool_bwd_quad_shapes(C, H, W):
    """maxpool backward (one thread per 2x2 input quad) on even and odd / non-square inputs."""
    N, Cc = 2, 64
    x = rnd(N, H, W, Cc, seed=21)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(N, OH, OW, Cc, dtype=BF, device=dev)
    am = torch.empty(N, OH, OW, Cc, dtype=torch.uint8, device=dev)
    C.maxpool_fwd(x, y, am)
    xr = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = F.max_pool2d(xr, 3, 2, 1)
    dy = rnd(N, OH, OW, Cc, seed=22)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    dx = torch.empty_like(x)
    C.maxpool_bwd(dy, am, dx)
    assert relerr(dx, xr.grad.permute(0, 2, 3, 1)) < 1e-2
    dx2 = torch.full_like(x, 7.0)
    C.maxpool_bwd(dy, am, dx2)  # every input element written, deterministically
    assert torch.equal(dx, dx2)


@pytest.mark.parametrize("B,NC", [(32, 1000), (5, 1000), (64, 100)])
def test_xent_wide_head_wave_rows(C, B, NC):
    """ResNet-width cross-entropy (one wave per row, last-block mean) vs fp32 PyTorch."""
    g = torch.Generator().manual_seed(B + NC)
    lg = (torch.randn(B, NC, generator=g) * 3).to(dev)
    y = torch.randint(0, NC, (B,), generator=g).to(dev)
    dl = torch.empty_like(lg)
    loss = torch.empty(1, device=dev)
    C.xent(lg, 1, None, y, None, dl, loss, None, 1.0 / B, 0.0)
    lr = lg.clone().requires_grad_(True)
    ref = F.cross_entropy(lr, y)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-4 * max(1.0, abs(ref.item()))
    assert relerr(dl, lr.grad) < 1e-4
    loss2 = torch.empty(1, device=dev)
    C.xent(lg, 1, None, y, None, dl, loss2, None, 1.0 / B, 0.0)
    assert torch.equal(loss, loss2)  # fixed-order row sum


def test_pools_and_head(C):
    N, H, Cc = 2, 9, 64
    x = rnd(N, H, H, Cc, seed=9)
    OH = (H - 1) // 2 + 1
    y = torch.empty(N, OH, OH, Cc, dtype=BF, device=dev)
    am = torch.empty(N, OH, OH, Cc, dtype=torch.uint8, device=dev)
    C.maxpool_fwd(x, y, am)
    xr = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = F.max_pool2d(xr, 3, 2, 1)
    assert torch.equal(y.float(), ref.detach().permute(0, 2, 3, 1))
    dy = rnd(N, OH, OH, Cc, seed=10)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    dx = torch.empty_like(x)
    C.maxpool_bwd(dy, am, dx)
    assert relerr(dx, xr.grad.permute(0, 2, 3, 1)) < 1e-2
    a = torch.empty(N, Cc, device=dev)
    C.avgpool_fwd(x, a)
    assert relerr(a, x.float().mean((1, 2))) < 1e-5
    w = torch.randn(1000, Cc, device=dev) * 0.05
    b = torch.randn(1000, device=dev)
    o = torch.empty(N, 1000, device=dev)
    C.sgemm(N, 1000, Cc, a, Cc, 1, w, 1, Cc, o, b, 1.0)
    assert relerr(o, a @ w.t() + b) < 1e-5


@pytest.mark.parametrize("side", [64, 72])
def test_resnet18_hip_vs_cpu_fp32(side):
    """Whole-network gradients of the HIP ResNet-18 vs an fp32 CPU oracle, at 64 x 64 images
    (layers 16, 8, 4, 2 wide) and 72 x 72 (18, 9, 5, 3: generic-width halo kernels, the halo
    weight gradient on two layers and its per-tap fallback on the other two, the parity-class
    data gradient from odd inputs, the max-pool from 36).

    A random-init ResNet-18 amplifies rounding through 20 BatchNorm backwards, so a
    fixed tolerance is meaningless: the bar is the precision floor, i.e. the error
    that torch's own bf16 CPU run of the same network shows against the same fp32
    oracle (scripts/debug_resnet.py prints both columns).  The HIP path must be no
    worse than that floor (plus a small slack) on every parameter."""
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss

    torch.manual_seed(0)
    cpu = resnet18(num_classes=10)
    cpu16 = resnet18(num_classes=10)
    cpu16.load_state_dict(cpu.state_dict())
    gpu = resnet18(num_classes=10).to(dev)
    gpu.load_state_dict(cpu.state_dict())
    x = torch.randn(4, 3, side, side)
    y = torch.randint(0, 10, (4,))
    lc = F.cross_entropy(cpu(x), y)
    lc.backward()
    cpu16 = cpu16.to(torch.bfloat16)
    F.cross_entropy(cpu16(x.to(torch.bfloat16)).float(), y).backward()
    lg = CrossEntropyLoss()(gpu(x.to(dev)), y.to(dev))
    lg.backward()
    assert abs(lg.item() - lc.item()) < 5e-2
    bad = []
    for (n, pc), (_, p16), (_, pg) in zip(cpu.named_parameters(), cpu16.named_parameters(),
                                          gpu.named_parameters()):
        e, floor = relerr(pg.grad, pc.grad), relerr(p16.grad.float(), pc.grad)
        if e > 1.25 * floor + 0.03:
            bad.append((n, e, floor))
    assert not bad, bad
    for (n, bc), (_, bg) in zip(cpu.named_buffers(), gpu.named_buffers()):
        if bc.dtype.is_floating_point:
            assert relerr(bg, bc) < 2e-2, n
        else:
            assert torch.equal(bg.cpu(), bc), n


def test_resnet18_direct_grads_and_bf16_weight_copy():
    """Flattened model (FusedSGD/DDP): the HIP Functions accumulate weight / BN / fc
    gradients straight into the flat .grad views and read the flat bf16 weight copy; the
    gradients equal the unflattened model's returned ones (bitwise, except the fc GEMM
    whose library kernel differs between addmm_ and mm), and the optimizer step leaves the
    bf16 copy fresh (rewritten in the update kernel, no rebuild)."""
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    torch.manual_seed(0)
    a = resnet18(num_classes=10).to(dev)
    b = resnet18(num_classes=10).to(dev)
    b.load_state_dict(a.state_dict())
    opt = FusedSGD(b, lr=0.1, momentum=0.9)
    fs = opt.flat
    x = torch.randn(4, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (4,), device=dev)
    CrossEntropyLoss()(a(x), y).backward()
    for it in range(2):
        opt.zero_grad()
        CrossEntropyLoss()(b(x), y).backward()
        if it == 0:
            for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
                assert pb.grad.data_ptr() == fs.view(fs.grads, n).data_ptr(), n
                if n.startswith("fc."):
                    assert torch.allclose(pa.grad, pb.grad, rtol=1e-4, atol=1e-6), n
                else:
                    assert torch.equal(pa.grad, pb.grad), n
        opt.step()
        assert fs._bf16_version == fs.params._version
        assert torch.equal(fs._bf16, fs.params.to(torch.bfloat16))
        # the stem's zero-padded bf16 weight (PAD4 shadow) is rewritten in the same pass
        pad_ref = F.pad(b.conv1.weight.detach().to(torch.bfloat16), (0, 1))
        assert len(fs._pad4) == 1
        assert torch.equal(next(iter(fs._pad4.values())), pad_ref)
    # a torch-side write to the parameters invalidates the copy; the next use rebuilds it
    with torch.no_grad():
        b.conv1.weight.mul_(0.5)
    assert fs._bf16_version != fs.params._version
    assert torch.equal(fs.bf16_view(b.conv1.weight), b.conv1.weight.to(torch.bfloat16))
    assert torch.equal(fs.bf16_pad4_view(b.conv1.weight),
                       F.pad(b.conv1.weight.detach().to(torch.bfloat16), (0, 1)))


@pytest.mark.parametrize("H", [112, 9])
def test_maxpool_reads_deferred_batchnorm_bitwise(C, H):
    """maxpool_fwd with the producer's BatchNorm + ReLU applied on load (BnAffine) ==
    bn_apply then maxpool: outputs and argmax bit for bit (ties and exact zeros included:
    channel 0 is all-zero after the ReLU)."""
    N, Cc = 2, 64
    yraw = rnd(N, H, H, Cc, seed=51)
    mean = torch.randn(Cc, device=dev) * 0.1
    invstd = torch.rand(Cc, device=dev) + 0.5
    gamma = torch.rand(Cc, device=dev) + 0.5
    beta = torch.randn(Cc, device=dev) * 0.3
    beta[0] = -100.0
    out = torch.empty_like(yraw)
    C.bn_apply(yraw, mean, invstd, gamma, beta, None, True, out)
    OH = (H - 1) // 2 + 1
    y0, y1 = (torch.empty(N, OH, OH, Cc, dtype=BF, device=dev) for _ in range(2))
    a0, a1 = (torch.empty(N, OH, OH, Cc, dtype=torch.uint8, device=dev) for _ in range(2))
    C.maxpool_fwd(out, y0, a0)
    C.maxpool_fwd(yraw, y1, a1, [mean, invstd, gamma, beta])
    assert torch.equal(y0, y1) and torch.equal(a0, a1)
    assert (y1[..., 0] == 0).all()


@pytest.mark.parametrize("N,H,Cin,Cout", [(4, 56, 64, 64), (4, 28, 128, 128), (8, 14, 256, 256), (8, 7, 512, 512)])
def test_halo_conv_reads_deferred_batchnorm_bitwise(C, N, H, Cin, Cout):
    """conv2 of a BasicBlock staging its input as the producer's BatchNorm + ReLU (BnAffine
    in the halo forward and the halo weight gradient) == bn_apply first: the forward output,
    its BatchNorm statistics and the weight gradient bit for bit; the zero padding stays 0."""
    xraw = rnd(N, H, H, Cin, seed=61)
    w = rnd(Cout, 3, 3, Cin, scale=0.05, seed=62)
    dy = rnd(N, H, H, Cout, scale=0.5, seed=63)
    mean = torch.randn(Cin, device=dev) * 0.1
    invstd = torch.rand(Cin, device=dev) + 0.5
    gamma = torch.rand(Cin, device=dev) + 0.5
    beta = torch.randn(Cin, device=dev) * 0.3
    bn = [mean, invstd, gamma, beta]
    xact = torch.empty_like(xraw)
    C.bn_apply(xraw, mean, invstd, gamma, beta, None, True, xact)
    outs = []
    for x, b in ((xact, None), (xraw, bn)):
        y = torch.empty(N, H, H, Cout, dtype=BF, device=dev)
        _, _, sp, rows, _, halo = C.conv_gemm_plan(x, y, 3, 3, 1, 1, False, 0, 0, 0, -1, 1)  # halo forced
        assert halo == 1
        stats = torch.empty(rows, 2, Cout, device=dev)
        part = torch.empty(sp * y.numel(), device=dev) if sp > 1 else None
        C.conv_gemm_fwd(x, w, None, y, 3, 3, 1, 1, False, stats, part, 0, 0, 0, 1, bn=b)
        ppc = C.conv_gemm_wgrad_ppc(x, dy, 3, 3, 1, 1)
        assert C.conv_gemm_wgrad_uses_halo(x, dy, 3, 3, 1, 1, ppc)
        ch = C.conv_gemm_wgrad_chunks(x, dy, 3, 3, 1, 1, ppc)
        row = Cout * 9 * Cin
        slab = torch.empty(ch, row, device=dev)
        C.conv_gemm_wgrad(dy, x, slab, 3, 3, 1, 1, ppc, False, bn=b)
        dw = torch.zeros(row, device=dev)
        C.grad_reduce([(slab, row, 0, row, ch, dw, 1.0, False)])
        torch.cuda.synchronize()
        outs.append((y, stats, dw))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_resnet18_deferred_stem_bn_bitwise(monkeypatch):
    """Every BatchNorm + ReLU without a residual add deferred into its consumer's loads (the
    stem's into the maxpool, each block's bn1 into conv2's halo forward / weight gradient; no
    bn_apply pass, the BN backward's mask recomputed from the conv output) trains
    bit-identically to the materialised chain: loss, every gradient and the BN running
    statistics."""
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, resnet_fn

    torch.manual_seed(0)
    base = resnet18(num_classes=10).to(dev)
    x = torch.randn(4, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (4,), device=dev)
    res = []
    for defer in (False, True):
        monkeypatch.setattr(resnet_fn, "DEFER_BN", defer)
        m = resnet18(num_classes=10).to(dev)
        m.load_state_dict(base.state_dict())
        loss = CrossEntropyLoss()(m(x), y)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters()},
                    {n: b.clone() for n, b in m.named_buffers()}))
    assert torch.equal(res[0][0], res[1][0])
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n
    for n in res[0][2]:
        assert torch.equal(res[0][2][n], res[1][2][n]), n


def test_graphed_step_equals_eager():
    """GraphedStep (whole training step in one hipGraph: forward, backward with direct
    gradients, FusedSGD with the bf16 weight copy, BN running stats) replays exactly the
    eager step: bitwise-equal parameters and buffers after the same number of steps."""
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    xs = [torch.randn(4, 3, 64, 64, device=dev) for _ in range(2)]
    ys = [torch.randint(0, 10, (4,), device=dev) for _ in range(2)]

    def make_step(model):
        opt = FusedSGD(model, lr=0.05, momentum=0.9, weight_decay=1e-4)
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return step

    torch.manual_seed(0)
    e = resnet18(num_classes=10).to(dev)
    f = resnet18(num_classes=10).to(dev)
    f.load_state_dict(e.state_dict())
    se, sf = make_step(e), make_step(f)
    order = [0, 0, 1, 0, 1]  # graphed: 2 warm-up steps on its static input (xs[0]), then replays
    for i in order:
        le = se(xs[i], ys[i])
    gf = GraphedStep(sf, (xs[0], ys[0]), warmup=2)
    for i in order[2:]:
        lf = gf(xs[i], ys[i])
    torch.cuda.synchronize()
    assert torch.equal(le, lf)
    for (n, pe), (_, pf) in zip(e.named_parameters(), f.named_parameters()):
        assert torch.equal(pe, pf), n
    for (n, be), (_, bf) in zip(e.named_buffers(), f.named_buffers()):
        assert torch.equal(be, bf), n


def test_image_gather_nhwc4_matches_cpu_pipeline():
    from ddp_amd.data import DeviceImages, synthetic_imagenet

    imgs, labels = synthetic_imagenet(12, 20, 7, seed=3)
    g, c = DeviceImages(imgs, labels, dev), DeviceImages(imgs, labels, "cpu")
    idx = torch.tensor([5, 0, 11, 5])
    xg, yg = g.gather(idx.to(dev))
    xc, yc = c.gather(idx)
    assert xg.dtype == BF and tuple(xg.shape) == (4, 20, 20, 4)
    assert torch.equal(xg[..., 3].float().cpu(), torch.zeros(4, 20, 20))
    assert torch.equal(xg[..., :3].float().cpu(), xc.permute(0, 2, 3, 1).to(BF).float())
    assert torch.equal(yg.cpu(), yc)


def _resnet_trainer_worker(rank, port, ckdir, graph, q):
    import os

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        from ddp_amd.engine.trainer import TrainOptions, ddp_train

        opts = TrainOptions(checkpoint_dir=ckdir, log_every=1, model="resnet18", image_size=64,
                            num_classes=10, dataset_size=40, momentum=0.9, graph_module=graph)
        model = ddp_train(rank, 1, 1, 8, opts)
        q.put(("ok", float(sum(p.double().sum() for p in model.parameters()))))
    except Exception as e:  # noqa: BLE001
        q.put((repr(e), None))


def test_resnet18_trainer_gpu_graph_equals_eager(tmp_path, capfd):
    """`train_ddp.py --model resnet18` on the GPU module path (RCCL PG of size 1): the
    graphed loop (--graph_module: warm-up step on batch 0, then replays, eager ragged
    tail) trains exactly like the eager loop, and writes the torchvision-layout checkpoint."""
    import torch.multiprocessing as mp

    from ddp_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    res = {}
    for graph in (False, True):
        q = ctx.Queue()
        p = ctx.Process(target=_resnet_trainer_worker,
                        args=(0, free_port(), str(tmp_path / f"ck{int(graph)}"), graph, q))
        p.start()
        res[graph] = q.get(timeout=240)
        p.join(timeout=60)
        assert res[graph][0] == "ok", res[graph]
    assert res[True][1] == res[False][1]
    out = capfd.readouterr().out
    assert "Epoch 0 | Batch 4 | Loss:" in out  # 40 images / batch 8: 5 steps, logged each step
    ck = torch.load(str(tmp_path / "ck1" / "epoch_0.pt"), weights_only=True)
    assert tuple(ck["model"]["conv1.weight"].shape) == (64, 3, 7, 7)


def test_linear_head_in_tree_gemm_matches_torch():
    """The classifier head runs on the in-tree fp32 GEMM (no library Cijk kernels): forward
    with the bias, dx, and dW / db accumulated into the flat gradient views."""
    from ddp_amd.ops.resnet_fn import linear_head

    g = torch.Generator().manual_seed(5)
    x = torch.randn(32, 512, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(1000, 512, generator=g) * 0.05).to(dev).requires_grad_(True)
    b = (torch.randn(1000, generator=g) * 0.1).to(dev).requires_grad_(True)
    out = linear_head(x, w, b)
    ref = x.detach().double() @ w.detach().double().t() + b.detach().double()
    assert ((out.double() - ref).norm() / ref.norm()).item() < 1e-6
    dl = torch.randn(32, 1000, generator=g).to(dev)
    out.backward(dl)
    d = dl.double()
    for got, want in ((x.grad, d @ w.detach().double()), (w.grad, d.t() @ x.detach().double()),
                      (b.grad, d.sum(0))):
        assert ((got.double() - want).norm() / want.norm()).item() < 1e-6


def test_residual_join_fused_into_producer_backward():
    """The residual branch's gradient is added inside the producer's backward (BatchNorm /
    maxpool backward load both upstream gradients): bitwise the same gradients as the
    plain autograd add, and no elementwise add kernel in the backward."""
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss
    from ddp_amd.ops import resnet_fn as R

    torch.manual_seed(0)
    a = resnet18(num_classes=10).to(dev)
    b = resnet18(num_classes=10).to(dev)
    b.load_state_dict(a.state_dict())
    x = torch.randn(4, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (4,), device=dev)
    CrossEntropyLoss()(a(x), y).backward()
    orig = R.attach_stash
    R.attach_stash = lambda t: None  # residual gradients through autograd's add instead
    try:
        CrossEntropyLoss()(b(x), y).backward()
    finally:
        R.attach_stash = orig
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa.grad, pb.grad), n
    a.zero_grad(set_to_none=True)  # (accumulating into existing .grad would add)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        CrossEntropyLoss()(a(x), y).backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert not any("CUDAFunctor_add" in n or n.startswith("Cijk") for n in names), \
        sorted({n for n in names if "add" in n.lower() or n.startswith("Cijk")})
