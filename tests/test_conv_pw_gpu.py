"""The pointwise convolution family (csrc/kernels/conv_pw.hip) per element on MI355X, the
Bottleneck block and ResNet-50 built on it.

Kernels against float64 on the same bf16 operands, bounds a priori (tests/test_resnet_geometry_gpu.py,
whose checkers are imported): bf16 outputs 2**-8 |ref| + 2 n u A, fp32 dW 2 n u A (n + 1 terms and
A + |prior| under accumulate), stats slab 2 P u S_abs from the stored bf16 y; the inference epilogue
takes tests/test_resnet_infer_gpu.py's bound.  Every output and slab is NaN-filled between sentinel
bands.  The AFF builds (a deferred BatchNorm + ReLU applied while staging) must equal, bit for bit,
the plain builds run on bn_apply's materialised output: that equality is the design claim.
P = 70 is one full 64-pixel tile plus a 6-pixel tail (and a partial 128 tile); Cin = 192 is an odd
number of K-steps through the double buffer; Cout = 192 only divides into 64-channel tiles, and the
two shapes with Cout = 128 carry the 128-wide tiles (128 -> 128 also the 128-wide weight-gradient
tiles).  Only (shape, tile) pairs the plans offer are cases: every case launches its kernel.
"""
import pytest
import torch
import torch.nn.functional as F

from elementwise import BF, Guarded, U, bitwise, f64, rnd
from test_resnet_geometry_gpu import ratio_bf16, ratio_f32, ratio_stats

pytestmark = pytest.mark.gpu
dev = "cuda"
SHAPES = [(2, 5, 7, ci, co) for ci in (64, 192) for co in (64, 192)] + [(2, 5, 7, 128, 128), (2, 5, 7, 192, 128),
                                                                         (1, 1, 1, 64, 64)]
TILES = [(128, 128), (128, 64), (64, 64)]
FWD = [(s, t) for s in SHAPES for t in TILES if s[4] % t[1] == 0]                     # (pixels x Cout) tiles
WGRAD = [(s, t) for s in SHAPES[:-1] for t in TILES if s[4] % t[0] == 0 and s[3] % t[1] == 0]  # (Cout x Cin), P = 70
_CASES = {}


def case(N, H, W, Cin, Cout):
    """Operands, a deferred affine for x, and the float64 references - once per shape."""
    key = (N, H, W, Cin, Cout)
    if key not in _CASES:
        c = _CASES[key] = type("Case", (), {})()
        c.P = N * H * W
        c.x = rnd(N, H, W, Cin, seed=1)  # signed: it doubles as a raw conv output under the affine
        c.w = rnd(Cout, 1, 1, Cin, scale=0.05, seed=2)
        c.dy = rnd(N, H, W, Cout, scale=0.5, seed=3)
        c.bn = [rnd(Cin, scale=0.3, seed=4, dtype=torch.float32), rnd(Cin, seed=5, dtype=torch.float32).abs() + 0.5,
                rnd(Cin, seed=6, dtype=torch.float32), rnd(Cin, scale=0.2, seed=7, dtype=torch.float32)]
        xd, wd, dyd = f64(c.x).reshape(c.P, Cin), f64(c.w).reshape(Cout, Cin), f64(c.dy).reshape(c.P, Cout)
        c.y_ref, c.y_abs = (xd @ wd.t()).reshape(N, H, W, Cout), (xd.abs() @ wd.abs().t()).reshape(N, H, W, Cout)
        c.dw_ref, c.dw_abs = (dyd.t() @ xd).reshape(-1), (dyd.abs().t() @ xd.abs()).reshape(-1)
    return _CASES[key]


def materialised(C, c):
    """bn_apply's stored relu(bn(x)), 64 channels at a time (its gate wants C / 8 to divide 256)."""
    parts = []
    for c0 in range(0, c.x.shape[-1], 64):
        xs = c.x[..., c0:c0 + 64].contiguous()
        parts.append(torch.empty_like(xs))
        C.bn_apply(xs, *[t[c0:c0 + 64].contiguous() for t in c.bn], None, True, parts[-1])
    return torch.cat(parts, dim=-1).contiguous()


def fwd(C, c, x, bp, bc, bn=None):
    ok, pbp, pbc, rows = C.conv_pw_plan(c.P, x.shape[-1], c.w.shape[0], bp, bc)
    assert ok and (not bp or (pbp, pbc) == (bp, bc))
    y, stats = Guarded(tuple(c.dy.shape), BF), Guarded((rows, 2, c.w.shape[0]), torch.float32)
    C.conv_pw_fwd(x, c.w, y.t, stats.t, bn, bp, bc)
    torch.cuda.synchronize()
    y.check("y"), stats.check("stats")
    return y.t, stats.t


@pytest.mark.parametrize("shape,tile", FWD + [(s, (0, 0)) for s in SHAPES])
def test_forward_and_stats(C, shape, tile):
    (N, H, W, Cin, Cout), (bp, bc) = shape, tile
    c = case(N, H, W, Cin, Cout)
    y, stats = fwd(C, c, c.x, bp, bc)
    what = f"pw fwd {(N, H, W, Cin, Cout)} tile {bp}x{bc}"
    print("PW_RATIO", what, ratio_bf16(y, c.y_ref, c.y_abs, Cin, what), ratio_stats(stats, y, what))
    y2 = Guarded(tuple(y.shape), BF)
    C.conv_pw_fwd(c.x, c.w, y2.t, None, None, bp, bc)  # the plain epilogue stores the same values
    assert bitwise(y2.t, y)[0] == 0 and y2.check("y plain") is None


@pytest.mark.parametrize("shape,tile", FWD)
def test_deferred_affine_is_bitwise_the_materialised_input(C, shape, tile):
    (N, H, W, Cin, Cout), (bp, bc) = shape, tile
    c = case(N, H, W, Cin, Cout)
    xm = materialised(C, c)
    ya, sa = fwd(C, c, c.x, bp, bc, c.bn)
    ym, sm = fwd(C, c, xm, bp, bc)
    assert bitwise(ya, ym)[0] == 0 and bitwise(sa, sm)[0] == 0
    assert not torch.equal(ya, fwd(C, c, c.x, bp, bc)[0])  # (the affine is not the identity)
    bm, bn_tile = (bp, bc) if (shape, tile) in WGRAD else (64, 64)  # the same tile as co x ci where it divides
    for ppc in (32, 0):  # 3 chunks (P = 70) and one
        da, dm = wgrad(C, c, c.x, bm, bn_tile, ppc, bn=c.bn), wgrad(C, c, xm, bm, bn_tile, ppc)
        assert bitwise(da[0], dm[0])[0] == 0 and (da[1] is None or bitwise(da[1], dm[1])[0] == 0)


def wgrad(C, c, x, bm, bn_tile, ppc, accum=False, prior=None, bn=None):
    """(dw, slab or None): the slab + grad_reduce route when the plan has several chunks."""
    Cin, Cout = x.shape[-1], c.dy.shape[-1]
    pbm, pbn, pppc, ch = C.conv_pw_wgrad_plan(c.P, Cin, Cout, bm, bn_tile, ppc)
    assert pbm and (not ppc or (pppc == ppc and ch == -(-c.P // ppc)))
    dw = Guarded((Cout * Cin,), torch.float32, prior)
    slab = None
    if ch == 1:
        C.conv_pw_wgrad(c.dy, x, dw.t, accum, bn, bm, bn_tile, ppc)
    else:
        slab = Guarded((ch, Cout * Cin), torch.float32)
        C.conv_pw_wgrad(c.dy, x, slab.t, False, bn, bm, bn_tile, ppc)
        C.grad_reduce([(slab.t, Cout * Cin, 0, Cout * Cin, ch, dw.t, 1.0, accum)])
        torch.cuda.synchronize()
        slab.check("slab")
        assert bool(torch.isfinite(slab.t).all()), "unwritten slab elements"
    torch.cuda.synchronize()
    dw.check("dw")
    return dw.t, (slab.t if slab else None)


@pytest.mark.parametrize("shape,tile", WGRAD)
def test_weight_gradient(C, shape, tile):
    (N, H, W, Cin, Cout), (bm, bn_tile) = shape, tile
    c = case(N, H, W, Cin, Cout)
    what = f"pw wgrad {(N, H, W, Cin, Cout)} tile {bm}x{bn_tile}"
    dw, slab = wgrad(C, c, c.x, bm, bn_tile, 32)  # P = 70: chunks of 32, 32 and a ragged 6
    assert slab.shape[0] == 3
    r3 = ratio_f32(dw, c.dw_ref, c.dw_abs, c.P, what + " 3 chunks")
    dw2, slab2 = wgrad(C, c, c.x, bm, bn_tile, 32)
    assert bitwise(slab2, slab)[0] == 0 and bitwise(dw2, dw)[0] == 0, "the slab path must be bitwise run to run"
    prior = rnd(Cout * Cin, seed=77, dtype=torch.float32)
    dwa, none = wgrad(C, c, c.x, bm, bn_tile, 0, accum=True, prior=prior)
    assert none is None
    ra = ratio_f32(dwa, f64(prior) + c.dw_ref, c.dw_abs + f64(prior).abs(), c.P + 1, what + " accumulate")
    r1 = ratio_f32(wgrad(C, c, c.x, bm, bn_tile, 0)[0], c.dw_ref, c.dw_abs, c.P, what + " one chunk")
    print("PW_RATIO", what, r3, ra, r1)


@pytest.mark.parametrize("res,relu", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("bp,bc", TILES)
def test_inference_epilogue(C, bp, bc, res, relu):
    from test_resnet_infer_gpu import affine

    c = case(2, 5, 7, 192, 128)
    sc, sh = affine(128, 9)
    rs = rnd(2, 5, 7, 128, scale=1.5, seed=8)
    y = Guarded((2, 5, 7, 128), BF)
    C.conv_pw_infer(c.x, c.w, sc, sh, rs if res else None, y.t, relu, bp, bc)
    torch.cuda.synchronize()
    y.check("infer y")
    scd, shd, rd = f64(sc), f64(sh), (f64(rs) if res else torch.zeros_like(c.y_ref))
    pre = c.y_ref * scd + shd + rd
    ref = torch.relu(pre) if relu else pre
    bound = (2.0 ** -8 * ref.abs() + (192 + 2) * U * scd.abs() * c.y_abs
             + 3 * U * ((c.y_ref * scd).abs() + shd.abs() + rd.abs()) + 1e-30)
    o = f64(y.t)
    assert bool(torch.isfinite(o).all()) and ((o - ref).abs() / bound).max().item() <= 1.0


def relerr(a, b):
    return ((a.double().cpu() - b.double()).norm() / b.double().norm().clamp_min(1e-12)).item()


@pytest.mark.parametrize("cin,width,stride", [(64, 64, 1), (256, 64, 1), (256, 128, 2)])
def test_bottleneck_forward_backward(cin, width, stride):
    """One Bottleneck (downsample, identity, stride 2) against the same block in float64 on the
    bf16-rounded parameters.  The bar is tests/test_resnet_gpu.py test_resnet18_hip_vs_cpu_fp32's:
    error <= 1.25 x floor + 0.03 per tensor, floor = torch's own bf16 CPU run of the block."""
    from ddp_amd.models.resnet import Bottleneck

    torch.manual_seed(0)
    ref = Bottleneck(cin, width, stride)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.to(BF).float())
    gpu, low = Bottleneck(cin, width, stride).to(dev), Bottleneck(cin, width, stride)
    gpu.load_state_dict(ref.state_dict()), low.load_state_dict(ref.state_dict())
    ref, low = ref.double(), low.to(BF)
    x = torch.relu(torch.randn(2, cin, 8, 8)).to(BF)
    g = torch.randn(2, 4 * width, 8 // stride, 8 // stride).to(BF)
    outs = []
    for blk, xi in ((ref, x.double()), (low, x.clone())):
        xi.requires_grad_(True)
        o = blk.forward_nchw(xi)
        o.backward(g.to(o.dtype))
        outs.append([o.detach(), xi.grad] + [p.grad for p in blk.parameters()])
    xg = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
    og = gpu.forward_hip(xg)
    og.backward(g.permute(0, 2, 3, 1).contiguous().to(dev))
    got = [og.detach().permute(0, 3, 1, 2), xg.grad.permute(0, 3, 1, 2)] + [p.grad for p in gpu.parameters()]
    names = ["out", "dx"] + [n for n, _ in gpu.named_parameters()]
    bad = [(n, relerr(a, r), relerr(lo, r)) for n, a, r, lo in zip(names, got, outs[0], outs[1])
           if relerr(a, r) > 1.25 * relerr(lo, r) + 0.03]
    assert not bad, bad


@pytest.fixture(scope="module")
def r50():
    """ResNet-50 with BatchNorm statistics and affines far from the identity (a wrong folded
    scale, shift or channel in an inference epilogue moves the logits)."""
    from ddp_amd.models import resnet50
    from test_resnet_eval_gpu import randomise_bn

    torch.manual_seed(0)
    return randomise_bn(resnet50(num_classes=16)).to(dev)


def test_resnet50_forward_infer(r50):
    """tests/test_resnet_eval_gpu.py's yardstick: the fused inference logits are no further from
    the float64 twin (bf16-rounded conv weights) than 1.5 x the eval-mode training forward's."""
    from ddp_amd.models import resnet50
    from ddp_amd.models.layers import Conv2d

    twin = resnet50(num_classes=16)
    twin.load_state_dict(r50.state_dict())
    with torch.no_grad():
        for m in twin.modules():
            if isinstance(m, Conv2d):
                m.weight.copy_(m.weight.to(BF).float())
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(BF)
    with torch.no_grad():
        ref = twin.double().eval()(x.double())
        fused = r50.forward_infer(x.float().to(dev))
        r50.eval()
        unfused = r50(x.float().to(dev)).float()
        r50.train()
    ef, eu = (f64(fused) - ref).abs().max().item(), (f64(unfused) - ref).abs().max().item()
    print(f"RESNET50_EVAL fused {ef:.5f} unfused {eu:.5f} max |logit| {ref.abs().max().item():.3f}")
    assert eu > 0 and ef <= 1.5 * eu


def test_resnet50_graphed_step_equals_eager(r50):
    """One whole training step captured in a graph (--graph_module's GraphedStep) replays bitwise
    the eager step: parameters and buffers, over several replays."""
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet50
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    x, y = torch.randn(2, 3, 64, 64, device=dev), torch.randint(0, 16, (2,), device=dev)
    nets = [resnet50(num_classes=16).to(dev) for _ in range(2)]
    steps = []
    for m in nets:
        m.load_state_dict(r50.state_dict())
        opt, lossf = FusedSGD(m, lr=0.05, momentum=0.9, weight_decay=1e-4), CrossEntropyLoss()

        def step(xi, yi, m=m, opt=opt, lossf=lossf):
            opt.zero_grad()
            loss = lossf(m(xi), yi)
            loss.backward()
            opt.step()
            return loss
        steps.append(step)
    for _ in range(4):
        le = steps[0](x, y)
    gs = GraphedStep(steps[1], (x, y), warmup=2)
    for _ in range(2):
        lg = gs(x, y)
    torch.cuda.synchronize()
    assert torch.equal(le, lg)
    for (n, a), (_, b) in zip(list(nets[0].named_parameters()) + list(nets[0].named_buffers()),
                              list(nets[1].named_parameters()) + list(nets[1].named_buffers())):
        assert torch.equal(a, b), n
