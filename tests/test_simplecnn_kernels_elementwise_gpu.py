"""SimpleCNN step kernels, the flat SGD and the slab reducer per element, on MI355X.

Every kernel of conv3x3.hip (forward, fused fc epilogue, data gradient, fused conv1 weight
gradient, weight gradient), conv1.hip, linear.hip, xent.hip's xent_rows and optim.hip is
compared with a float64 CPU reference of the same operation (ddp_amd/ops/reference.py, held
against torch's double-precision operators by tests/test_simplecnn_kernel_bounds_cpu.py),
computed from exactly the tensors the kernel reads (masks from the stored activations,
gradients from the stored values), element by element, against an a-priori rounding bound
(ddp_amd/ops/kernel_bounds.py).  Nothing is calibrated on the kernels.

u = 2**-24, n = accumulated terms, A = the operation on absolute values.

    fp32 outputs / slabs, bf16 operands (exact products)    E = 2 n u A
    exact-fp32 builds (the products round too)              E = 3 n u A
    bf16 outputs                                            2**-8 (|ref| + E) + E

Terms counted from the kernels:
  conv3x3_fwd      n = 9 Cin + 1 (the MFMA chain over taps and input channels, the bias add)
  fused fc         n = 64 CH + CH / 4: a block's CH = 64 pxt pixels x 64 channels of the STORED
                   activation against the fc weight (v_dot2c / fma chain), the 16-lane sums and
                   the fixed-order sum over the block's CH / 16 tiles x 4 channel groups
  conv3x3_dgrad    n = 9 Cout; masked elements are exactly 0
  fused conv1 wgrad  per block: n = CH + 9 (an fma per pixel of the stored dZ1 against x, x = u8 / 255
                   rounds once, 16-lane sum, 4 waves)
  conv3x3_wgrad    per slab row: n = nslot = roundup32(R roundup8(W)) pixel slots (the K dimension
                   the MFMAs run over, padding included), bias = the same chain against ones;
                   reduced gradient: the rows' bounds plus the reducer's 2 (rows + 2) u sum |row|
  conv1_fwd        n = 10 (9 fma and the bias), 11 with the uint8 input's / 255
  conv1_wgrad      n = chunk (+ 1 with uint8)
  fc_partial       per 16-pixel tile n = 16 C + 6 (the lanes' fma chains, the wave sum); fc_reduce from
                   the partials it reads n = HW / 16 + 1; the logits end to end n = HW C + HW / 16 + 1
  fc_bwd         : dX n = NO, dW / dbias n = B + 2 (the scale),
                   loss n = B + 1
  xent_rows        the bound of tests/test_resnet_ops_elementwise_gpu.py with the logit's own
                   error e_l = 2 G u (sum |part| + |bias|), G = partials per logit + the bias:
                   |dl - ref| <= g (p (2 D + 64) u + 2 p e_l + 2 u); the row loss is evaluated as
                   (mx + log se) - x[label], which rounds at the logits' magnitude:
                   (D + 64) u max(1, |ref|) + 2 e_l + 2 u (|mx| + |x_label|)
  sgd              kernel_bounds.sgd_bounds: 6 u P, 4 u BUF (sgd_one's fma roundings)
  grad_reduce      2 (rows + 2) u (|scale| sum |row| + |prior|), and bit-identical to the float32
                   replay of slab_reduce.h's order

Every output, slab and workspace is carved out of a larger buffer with sentinel bands on both
sides and pre-filled with NaN.  Run with -s for the KERN_RATIO <family> <shape> <error / bound>
lines; profiles/simplecnn_kernels/README.md records the largest per family and shape.
"""
import numpy as np
import pytest
import torch

from ddp_amd.ops import kernel_bounds as K
from ddp_amd.ops import reference as R
from ddp_amd.ops.functional import fc_weight_frag
from ddp_amd.ops.kernel_bounds import acc_bound, bf16_store_bound, ratio
from elementwise import BF, F32, SENTINEL, Guarded, U, bits, f64, n32, report_ratio, rnd
from engine_step_cases import fold_terms, wgrad_nslot, wgrad_rows_of

pytestmark = pytest.mark.gpu
dev = "cuda"
LDS_MAX = 160 * 1024


def out_bound(ref, E, dtype):
    return bf16_store_bound(ref, E) if dtype == BF else E


# ------------------------------------------------------------------ LDS budgets (conv3x3.hip)
def fwd_lds(W, Cin, pxt, es):
    XR, pad = 64 * pxt + 2 * W + 2, 16 if es == 2 else 8
    b = es * (64 * (9 * Cin + pad) + XR * (Cin + pad))
    return ((b + 15) & ~15) + 4 * 4 * pxt * 4 * 16


def dgrad_lds(W, Cout, pxt, es):
    XR, pad = 64 * pxt + 2 * W + 2, 16 if es == 2 else 8
    return es * (32 * (9 * Cout + pad) + XR * (Cout + pad))


def wgrad_lds(W, Cin, Cout, Rr, es):
    Wp = (W + 7) & ~7
    nslot = (Rr * Wp + 31) // 32 * 32
    return es * (nslot * (Cout + 16) + (Rr + 2) * (Wp + 2) * (Cin + 16))


# --------------------------------------------------------------------------- conv3x3 cases
SPEC = (28, 28, 32, 64)
GENERIC = [(5, 7, 32, 64), (6, 12, 64, 128), (4, 40, 32, 64), (12, 12, 32, 64)]
# 6 x 12 x 64 -> 128 exceeds the exact-fp32 forward / data-gradient LDS budgets (the binding refuses,
# asserted below); these two fit and give the fp32 builds their grid.y = 2 (Cout / 64, Cin / 32)
GENERIC_FWD = GENERIC + [(6, 12, 32, 128)]
GENERIC_DGRAD = GENERIC + [(6, 12, 64, 64)]
DT = [pytest.param(BF, id="bf16"), pytest.param(F32, id="fp32")]


def conv_inputs(B, H, W, Cin, Cout, dtype, seed=100):
    x = rnd(B, H, W, Cin, relu=True, seed=seed, dtype=dtype)
    w = rnd(Cout, 3, 3, Cin, scale=0.1, seed=seed + 1, dtype=dtype)
    b = rnd(Cout, scale=0.1, seed=seed + 2, dtype=F32)
    return x, w, b


def run_fwd(C, B, H, W, Cin, Cout, dtype, pxt, relu, family):
    es = 2 if dtype == BF else 4
    x, w, b = conv_inputs(B, H, W, Cin, Cout, dtype)
    y = Guarded((B, H, W, Cout), dtype)
    what = f"conv3x3_fwd {(B, H, W, Cin, Cout)} {dtype} pxt={pxt} relu={relu}"
    if fwd_lds(W, Cin, pxt, es) > LDS_MAX:
        with pytest.raises(RuntimeError, match="LDS"):
            C.conv3x3_fwd(x, w, b, y.t, relu, None, None, 0, pxt)
        return
    C.conv3x3_fwd(x, w, b, y.t, relu, None, None, 0, pxt)
    torch.cuda.synchronize()
    ref = R.conv3x3_64(x, w, b, relu)
    A = R.conv3x3_64(x.abs(), w.abs(), b.abs())
    E = acc_bound(9 * Cin + 1, A, dtype == F32)
    ratio(family, (B, H, W, Cin, Cout, pxt), y.t, ref, out_bound(ref, E, dtype), what)
    if relu:
        assert bool((f64(y.t) >= 0).all()), f"{what}: negative ReLU output"
    y.check(what)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("pxt", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_fwd_specialised(C, B, pxt, relu, dtype):
    run_fwd(C, B, *SPEC, dtype, pxt, relu, "fwd_spec_" + ("bf16" if dtype == BF else "fp32"))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W,Cin,Cout", GENERIC_FWD)
def test_conv3x3_fwd_generic(C, H, W, Cin, Cout, B, dtype):
    """Every (pxt, relu) template branch of the generic build."""
    for pxt, relu in ((1, True), (1, False), (2, True), (2, False)):
        run_fwd(C, B, H, W, Cin, Cout, dtype, pxt, relu, "fwd_gen_" + ("bf16" if dtype == BF else "fp32"))


def run_fwd_fc(C, B, H, W, dtype, pxt, family):
    Cin, Cout, NO, HW, CH = 32, 64, 10, H * W, 64 * pxt
    x, w, b = conv_inputs(B, H, W, Cin, Cout, dtype, seed=110)
    wfc = rnd(NO, HW, Cout, scale=0.05, seed=113, dtype=dtype)
    nblk = C.conv3x3_dgrad_blocks(B, H, W, pxt)
    y, part = Guarded((B, H, W, Cout), dtype), Guarded((nblk, 2, NO), F32)
    C.conv3x3_fwd(x, w, b, y.t, True, fc_weight_frag(wfc, HW, Cout, dtype), part.t, NO, pxt)
    torch.cuda.synchronize()
    what = f"conv3x3_fwd+fc {(B, H, W)} {dtype} pxt={pxt}"
    ref = R.conv3x3_64(x, w, b, True)
    E = acc_bound(9 * Cin + 1, R.conv3x3_64(x.abs(), w.abs(), b.abs()), dtype == F32)
    ratio(family + "_y", (B, H, W, pxt), y.t, ref, out_bound(ref, E, dtype), what)
    # the partial logits before any fold, from the activation the kernel stored
    pref = R.fc_block_partials64(y.t, wfc, CH)
    pA = R.fc_block_partials64(y.t.abs(), wfc.abs(), CH)
    ratio(family + "_part", (B, H, W, pxt), part.t, pref, acc_bound(64 * CH + CH // 4, pA, dtype == F32), what)
    # a slot whose image the block does not touch (or that lies past the batch) is +0.0
    got = part.t.cpu()
    for k in range(nblk):
        n0 = k * CH // HW
        last = (min((k + 1) * CH, B * HW) - 1) // HW
        if last == n0:
            assert bool((got[k, 1] == 0).all()) and not bool(torch.signbit(got[k, 1]).any()), f"{what}: block {k} slot 1"
    y.check(what)
    part.check(what)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("pxt", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_fwd_fused_fc_specialised(C, B, pxt, dtype):
    run_fwd_fc(C, B, 28, 28, dtype, pxt, "fwd_fc_spec_" + ("bf16" if dtype == BF else "fp32"))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("pxt", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
def test_conv3x3_fwd_fused_fc_generic(C, B, pxt, dtype):
    """12 x 12: an image holds a block (144 >= 128 pixels), blocks straddle images at B = 2."""
    run_fwd_fc(C, B, 12, 12, dtype, pxt, "fwd_fc_gen_" + ("bf16" if dtype == BF else "fp32"))


@pytest.mark.parametrize("H,W,pxt", [(4, 4, 1), (4, 8, 1), (8, 8, 2), (4, 12, 1), (7, 16, 2)])
def test_conv3x3_fwd_fused_fc_refuses_images_smaller_than_a_block(C, H, W, pxt):
    """The [blocks][2][10] partials hold two images per block; a block of 64 pxt pixels over
    images of fewer pixels spans three or more and the kernel would drop their logits.  The
    binding refuses before any launch (the outputs keep their NaN fill)."""
    B, HW = 5, H * W
    x, w, b = conv_inputs(B, H, W, 32, 64, BF)
    wfc = rnd(10, HW, 64, scale=0.05, seed=3)
    y = Guarded((B, H, W, 64), BF)
    part = Guarded((C.conv3x3_dgrad_blocks(B, H, W, pxt), 2, 10), F32)
    with pytest.raises(RuntimeError, match="must hold a block"):
        C.conv3x3_fwd(x, w, b, y.t, True, fc_weight_frag(wfc, HW, 64), part.t, 10, pxt)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all()) and bool(torch.isnan(part.t).all())


# ---------------------------------------------------------------------------- data gradient
def run_dgrad(C, B, H, W, Cin, Cout, dtype, pxt, mask_dy, mask_x, family):
    es = 2 if dtype == BF else 4
    dy = rnd(B, H, W, Cout, scale=0.5, seed=120, dtype=dtype)
    yact = rnd(B, H, W, Cout, seed=121, relu=True, dtype=dtype)
    xact = rnd(B, H, W, Cin, seed=122, relu=True, dtype=dtype)
    w = rnd(Cout, 3, 3, Cin, scale=0.1, seed=123, dtype=dtype)
    wt = w.view(Cout, 9, Cin).permute(1, 2, 0).contiguous()
    dx = Guarded((B, H, W, Cin), dtype)
    args = (dy, yact if mask_dy else None, wt, xact if mask_x else None, dx.t, pxt)
    what = f"conv3x3_dgrad {(B, H, W, Cin, Cout)} {dtype} pxt={pxt} mask_dy={mask_dy} mask_x={mask_x}"
    if dgrad_lds(W, Cout, pxt, es) > LDS_MAX:
        with pytest.raises(RuntimeError, match="LDS"):
            C.conv3x3_dgrad(*args)
        return
    C.conv3x3_dgrad(*args)
    torch.cuda.synchronize()
    g = f64(dy) * (f64(yact) > 0) if mask_dy else f64(dy)
    ref, A = R.conv3x3_dgrad64(g, w), R.conv3x3_dgrad64(g.abs(), w.abs())
    if mask_x:
        keep = f64(xact) > 0
        ref, A = ref * keep, A * keep
        assert bool((f64(dx.t)[~keep] == 0).all()), f"{what}: a masked element is not exactly 0"
    E = acc_bound(9 * Cout, A, dtype == F32)
    ratio(family, (B, H, W, Cin, Cout, pxt), dx.t, ref, out_bound(ref, E, dtype), what)
    dx.check(what)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("mask_dy,mask_x", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("pxt", [1, 2])
def test_conv3x3_dgrad_specialised(C, pxt, mask_dy, mask_x, dtype):
    run_dgrad(C, 3, *SPEC, dtype, pxt, mask_dy, mask_x, "dgrad_spec_" + ("bf16" if dtype == BF else "fp32"))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W,Cin,Cout", GENERIC_DGRAD)
def test_conv3x3_dgrad_generic(C, H, W, Cin, Cout, B, dtype):
    """Every (pxt, mask_dy, mask_x) template branch of the generic build."""
    for pxt, mdy, mx in [(p_, a_, b_) for p_ in (1, 2) for a_ in (False, True) for b_ in (False, True)]:
        run_dgrad(C, B, H, W, Cin, Cout, dtype, pxt, mdy, mx, "dgrad_gen_" + ("bf16" if dtype == BF else "fp32"))


@pytest.mark.parametrize("pxt", [1, 2])
@pytest.mark.parametrize("B,H,W", [(3, 28, 28), (2, 5, 7), (2, 12, 12), (1, 4, 40)])
def test_conv3x3_dgrad_fused_w1(C, B, H, W, pxt):
    """dZ1 and both conv1 slab segments of the fused data gradient (bf16, uint8 images
    through an index list with an offset), at the specialised geometry and - the binding
    accepts any H, W with Cin == 32 - at generic ones, both block sizes."""
    CH = 64 * pxt
    g0 = torch.Generator().manual_seed(130)
    data = torch.randint(0, 256, (40, H, W), generator=g0, dtype=torch.uint8).to(dev)
    idx = torch.randperm(40, generator=g0)[:B + 4].to(torch.int32).to(dev)
    dy = rnd(B, H, W, 64, scale=0.5, seed=131)
    a1 = rnd(B, H, W, 32, seed=132, relu=True)
    w = rnd(64, 3, 3, 32, scale=0.1, seed=133)
    wt = w.view(64, 9, 32).permute(1, 2, 0).contiguous()
    nblk = C.conv3x3_dgrad_blocks(B, H, W, pxt)
    dz1, slab = Guarded((B, H, W, 32), BF), Guarded((nblk, 320), F32)
    C.conv3x3_dgrad_fused_w1(dy, wt, a1, dz1.t, data, idx, None, 0, 4, slab.t, pxt)
    torch.cuda.synchronize()
    what = f"conv3x3_dgrad_fused_w1 {(B, H, W)} pxt={pxt}"
    keep = f64(a1) > 0
    ref = R.conv3x3_dgrad64(dy, w) * keep
    E = acc_bound(9 * 64, R.conv3x3_dgrad64(dy.abs(), w.abs()) * keep)
    ratio("dgrad_w1_dz1", (B, H, W, pxt), dz1.t, ref, bf16_store_bound(ref, E), what)
    assert bool((f64(dz1.t)[~keep] == 0).all())
    xs = data[idx[4:4 + B].long()].cpu()
    rw, rb, aw, ab = [], [], [], []
    for k in range(nblk):  # each slab row from the stored dZ1 of the block's own pixels
        px = (k * CH, min((k + 1) * CH, B * H * W))
        dwk, dbk = R.conv1_wgrad64(dz1.t, xs, px)
        awk, abk = R.conv1_wgrad64(dz1.t.abs(), xs, px)
        rw.append(dwk.reshape(-1)); rb.append(dbk); aw.append(awk.reshape(-1)); ab.append(abk)
    ref_slab = torch.cat([torch.stack(rw), torch.stack(rb)], 1)
    A_slab = torch.cat([torch.stack(aw), torch.stack(ab)], 1)
    ratio("dgrad_w1_slab", (B, H, W, pxt), slab.t, ref_slab, acc_bound(CH + 9, A_slab), what)
    gw, gb = Guarded((288,), F32), Guarded((32,), F32)
    C.grad_reduce([(slab.t, 320, 0, 288, nblk, gw.t, 1.0), (slab.t, 320, 288, 32, nblk, gb.t, 1.0)])
    torch.cuda.synchronize()
    red = K.reduce_bound(f64(slab.t), 1.0)
    tot = acc_bound(CH + 9, A_slab).sum(0) + red
    ratio("dgrad_w1_dw", (B, H, W, pxt), gw.t, ref_slab[:, :288].sum(0), tot[:288], what)
    ratio("dgrad_w1_db", (B, H, W, pxt), gb.t, ref_slab[:, 288:].sum(0), tot[288:], what)
    for g_ in (dz1, slab, gw, gb):
        g_.check(what)


# -------------------------------------------------------------------------- weight gradient
def run_wgrad(C, B, H, W, Cin, Cout, dtype, Rr, masked, family):
    es = 2 if dtype == BF else 4
    dy = rnd(B, H, W, Cout, scale=0.5, seed=140, dtype=dtype)
    yact = rnd(B, H, W, Cout, seed=141, relu=True, dtype=dtype)
    x = rnd(B, H, W, Cin, seed=142, relu=True, dtype=dtype)
    nblk = C.conv3x3_wgrad_blocks(B, H, Rr)
    assert nblk == B * -(-H // Rr)
    nw, row = Cout * 9 * Cin, Cout * 9 * Cin + Cout
    slab = Guarded((nblk, row), F32)
    what = f"conv3x3_wgrad {(B, H, W, Cin, Cout)} {dtype} R={Rr} masked={masked}"
    if wgrad_lds(W, Cin, Cout, Rr, es) > LDS_MAX:
        with pytest.raises(RuntimeError, match="LDS"):
            C.conv3x3_wgrad(dy, yact if masked else None, x, slab.t, Rr)
        return
    C.conv3x3_wgrad(dy, yact if masked else None, x, slab.t, Rr)
    torch.cuda.synchronize()
    g = f64(dy) * (f64(yact) > 0) if masked else f64(dy)
    ref, A = wgrad_rows_of(g, x, Rr), wgrad_rows_of(g.abs(), x.abs(), Rr)
    E = acc_bound(wgrad_nslot(W, Rr), A, dtype == F32)
    shape = (B, H, W, Cin, Cout, Rr)
    ratio(family + "_slab", shape, slab.t, ref, E, what)
    gw, gb = Guarded((nw,), F32), Guarded((Cout,), F32)
    C.grad_reduce([(slab.t, row, 0, nw, nblk, gw.t, 1.0), (slab.t, row, nw, Cout, nblk, gb.t, 1.0)])
    torch.cuda.synchronize()
    tot = E.sum(0) + K.reduce_bound(f64(slab.t), 1.0)
    ratio(family + "_dw", shape, gw.t, ref[:, :nw].sum(0), tot[:nw], what)
    ratio(family + "_db", shape, gb.t, ref[:, nw:].sum(0), tot[nw:], what)
    # the reducer itself: bit-identical to the float32 replay of slab_reduce.h's order
    GR = K.reduce_groups([nblk])
    rows32 = slab.t.cpu().numpy()
    assert np.array_equal(gw.t.cpu().numpy().view(np.int32), K.replay_reduce(rows32[:, :nw], GR).view(np.int32)), what
    assert np.array_equal(gb.t.cpu().numpy().view(np.int32), K.replay_reduce(rows32[:, nw:], GR).view(np.int32)), what
    for g_ in (slab, gw, gb):
        g_.check(what)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("Rr", [1, 2, 5, 7])
@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_wgrad_specialised(C, B, Rr, masked, dtype):
    """R = 5 leaves a 3-row last chunk; R = 1, 2 are what wgrad_rows picks for small batches."""
    run_wgrad(C, B, *SPEC, dtype, Rr, masked, "wgrad_spec_" + ("bf16" if dtype == BF else "fp32"))


def test_conv3x3_wgrad_128_rows(C):
    """B = 32 at R = 7: 128 slab rows, the 16-group reducer."""
    assert K.reduce_groups([32 * 4]) == 16
    run_wgrad(C, 32, *SPEC, BF, 7, True, "wgrad_spec_bf16_b32")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W,Cin,Cout,Rs", [(5, 7, 32, 64, (2, 5)), (6, 12, 64, 128, (4, 6)), (4, 40, 32, 64, (3, 1)),
                                             (12, 12, 32, 64, (5, 12))])
def test_conv3x3_wgrad_generic(C, H, W, Cin, Cout, Rs, B, dtype):
    """Each geometry at an R that does not divide H and one that does; W = 7, 12 pad the LDS
    rows to Wp = 8, 16; 64 -> 128 runs grid.y = 4."""
    for i, Rr in enumerate(Rs):
        run_wgrad(C, B, H, W, Cin, Cout, dtype, Rr, i == 0, "wgrad_gen_" + ("bf16" if dtype == BF else "fp32"))


# ----------------------------------------------------------------------------------- conv1
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B", [1, 3])
def test_conv1_fwd(C, B, dtype):
    H = W = 28
    g0 = torch.Generator().manual_seed(150)
    w = (torch.randn(32, 9, generator=g0) * 0.3).to(dev)
    b = (torch.randn(32, generator=g0) * 0.1).to(dev)
    xf = torch.rand(B, H, W, generator=g0).to(dev)
    data = torch.randint(0, 256, (50, H, W), generator=g0, dtype=torch.uint8).to(dev)
    idx = torch.randperm(50, generator=g0)[:B + 3].to(torch.int32).to(dev)
    tag = "bf16" if dtype == BF else "fp32"
    for name, xin, call, nterm in (
            ("float", xf, lambda y: C.conv1_fwd(xf, None, None, 0, 0, w, b, y, B, H, W), 10),
            ("u8", data[idx[3:3 + B].long()], lambda y: C.conv1_fwd(data, idx, None, 0, 3, w, b, y, B, H, W), 11)):
        y = Guarded((B, H, W, 32), dtype)
        call(y.t)
        torch.cuda.synchronize()
        what = f"conv1_fwd B={B} {name} {tag}"
        ref = R.conv1_64(xin, w, b)
        xa = f64(xin) / 255.0 if xin.dtype == torch.uint8 else f64(xin)
        A = R.conv3x3_64(xa.unsqueeze(-1), f64(w).abs().reshape(32, 3, 3, 1), f64(b).abs())
        E = acc_bound(nterm, A)
        ratio(f"conv1_fwd_{name}_{tag}", (B, H, W), y.t, ref, out_bound(ref, E, dtype), what)
        assert bool((f64(y.t) >= 0).all())
        y.check(what)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("chunk", [196, 256])
@pytest.mark.parametrize("B", [1, 3])
def test_conv1_wgrad(C, B, chunk, dtype):
    """chunk = 196 divides B * 784, 256 does not (a partial last block)."""
    H = W = 28
    g0 = torch.Generator().manual_seed(160)
    xf = torch.rand(B, H, W, generator=g0).to(dev)
    data = torch.randint(0, 256, (50, H, W), generator=g0, dtype=torch.uint8).to(dev)
    idx = torch.randperm(50, generator=g0)[:B + 2].to(torch.int32).to(dev)
    dy = rnd(B, H, W, 32, scale=0.5, seed=161, dtype=dtype)
    yact = rnd(B, H, W, 32, seed=162, relu=True, dtype=dtype)
    nblk = C.conv1_wgrad_blocks(B, H, W, chunk)
    tag = "bf16" if dtype == BF else "fp32"
    dz = f64(dy) * (f64(yact) > 0)
    for name, xin, nterm in (("float", xf, chunk), ("u8", data[idx[2:2 + B].long()], chunk + 1)):
        slab = Guarded((nblk, 320), F32)
        if name == "float":
            C.conv1_wgrad(xf, None, None, 0, 0, dy, yact, slab.t, B, H, W, 32, chunk)
        else:
            C.conv1_wgrad(data, idx, None, 0, 2, dy, yact, slab.t, B, H, W, 32, chunk)
        torch.cuda.synchronize()
        what = f"conv1_wgrad B={B} chunk={chunk} {name} {tag}"
        ref, A = [], []
        for k in range(nblk):
            px = (k * chunk, min((k + 1) * chunk, B * H * W))
            dwk, dbk = R.conv1_wgrad64(dz, xin.cpu(), px)
            awk, abk = R.conv1_wgrad64(dz.abs(), xin.cpu(), px)
            ref.append(torch.cat([dwk.reshape(-1), dbk])); A.append(torch.cat([awk.reshape(-1), abk]))
        ref, A = torch.stack(ref), torch.stack(A)
        ratio(f"conv1_wgrad_{name}_{tag}", (B, chunk), slab.t, ref, acc_bound(nterm, A, dtype == F32), what)
        slab.check(what)


# ----------------------------------------------------------------------------- fc and loss
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B", [1, 3])
def test_fc_partial_reduce(C, B, dtype):
    H = W = 28
    HW, Cc, NO = H * W, 64, 10
    x = rnd(B, H, W, Cc, relu=True, seed=170, dtype=dtype)
    wfc = rnd(NO, HW, Cc, scale=0.05, seed=171, dtype=dtype)
    bfc = rnd(NO, scale=0.1, seed=172, dtype=F32)
    part, out = Guarded((B, HW // 16, NO), F32), Guarded((B, NO), F32)
    C.fc_partial(x, wfc, part.t)
    C.fc_reduce(part.t, bfc, out.t, B, HW // 16, NO)
    torch.cuda.synchronize()
    tag = "bf16" if dtype == BF else "fp32"
    what = f"fc_partial+reduce B={B} {tag}"
    xt, wt = f64(x).reshape(B, HW // 16, 16 * Cc), f64(wfc).reshape(NO, HW // 16, 16 * Cc)
    pref = torch.einsum("bgk,ogk->bgo", xt, wt)
    pA = torch.einsum("bgk,ogk->bgo", xt.abs(), wt.abs())
    ratio(f"fc_partial_{tag}", (B,), part.t, pref, acc_bound(16 * Cc + 6, pA, dtype == F32), what)
    # fc_reduce from the partials it read: G sequential adds and the bias
    ref = f64(part.t).sum(1) + f64(bfc)
    ratio(f"fc_reduce_{tag}", (B,), out.t, ref, acc_bound(HW // 16 + 1, f64(part.t).abs().sum(1) + f64(bfc).abs()), what)
    # and end to end against the float64 fc of the inputs
    ref, A = R.fc64(x, wfc, bfc), R.fc64(x.abs(), wfc.abs(), bfc.abs())
    ratio(f"fc_logits_{tag}", (B,), out.t, ref, acc_bound(HW * Cc + HW // 16 + 1, A, dtype == F32), what)
    part.check(what)
    out.check(what)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("B", [1, 3])
def test_fc_bwd(C, B, mask, dtype):
    H = W = 28
    HW, Cc, NO, scale = H * W, 64, 10, 0.37
    x = rnd(B, H, W, Cc, relu=True, seed=180, dtype=dtype)
    wfc = rnd(NO, HW, Cc, scale=0.05, seed=181, dtype=dtype)
    dl = rnd(B, NO, scale=0.1, seed=182, dtype=F32)
    rows = rnd(B, seed=183, dtype=F32).abs() + 0.5
    dx, dw = Guarded((B, H, W, Cc), dtype), Guarded((NO, HW, Cc), F32)
    db, loss = Guarded((NO,), F32), Guarded((3,), F32)
    C.fc_bwd(dl, x, wfc, dx.t, dw.t, scale, mask, db.t, rows, loss.t)
    torch.cuda.synchronize()
    tag = "bf16" if dtype == BF else "fp32"
    what = f"fc_bwd B={B} mask={mask} {tag}"
    s32 = float(np.float32(scale))  # the binding narrows the double
    rdx, rdw, rdb = R.fc_bwd64(dl, x, wfc, s32, mask)
    adx, adw, adb = R.fc_bwd64(dl.abs(), x.abs() if not mask else x, wfc.abs(), s32, mask)
    f32b = dtype == F32
    Edx = acc_bound(NO, adx, f32b)
    ratio(f"fc_bwd_dx_{tag}", (B, mask), dx.t, rdx, out_bound(rdx, Edx, dtype), what)
    if mask:
        assert bool((f64(dx.t)[~(f64(x) > 0)] == 0).all()), f"{what}: a masked element is not exactly 0"
    ratio(f"fc_bwd_dw_{tag}", (B, mask), dw.t, rdw, acc_bound(B + 2, adw, f32b), what)
    ratio(f"fc_bwd_dbias_{tag}", (B, mask), db.t, rdb, acc_bound(B + 2, adb), what)
    lref = f64(rows).mean().reshape(1)
    ratio(f"fc_bwd_loss_{tag}", (B, mask), loss.t[:1], lref, acc_bound(B + 1, f64(rows).abs().mean().reshape(1)), what)
    assert bool(torch.isnan(loss.t[1:]).all()), f"{what}: wrote past loss_out[0]"
    for g_ in (dx, dw, db, loss):
        g_.check(what)


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("CH", [64, 128])
@pytest.mark.parametrize("B", [1, 3, 7])
def test_xent_rows(C, B, CH, with_idx):
    HW, NO = 784, 10
    nblk = -(-B * HW // CH)
    g0 = torch.Generator().manual_seed(190 + B)
    part_h = torch.randn(nblk, 2, NO, generator=g0) * 0.7
    bias_h = torch.randn(NO, generator=g0) * 0.1
    bias_h[5] = bias_h[2]
    terms = [fold_terms(b, CH, HW) for b in range(B)]
    # row 0: logits about 30 apart; the last row: two tied maxima (exactly)
    k0, s0 = terms[0][0]
    part_h[k0, s0, 0] += 15.0
    part_h[k0, s0, 9] -= 15.0
    if B > 1:
        for k, s in terms[B - 1]:
            part_h[k, s] = 0.0
        k, s = terms[B - 1][0]
        part_h[k, s] = torch.tensor([0.25, -1.0, 1.5, 0.5, -0.75, 1.5, 0.0, -2.0, 1.0, 0.125])
    labels_h = torch.randint(0, NO, (B + 5,), generator=g0).to(torch.int32)
    idx_h = torch.randperm(B + 5, generator=g0)[:B].to(torch.int32)
    gscale = float(np.float32(1.0 / B))
    part, bias = part_h.to(dev), bias_h.to(dev)
    dl, rows = Guarded((B, NO), F32), Guarded((B,), F32)
    C.xent_rows(part, HW, CH, bias, labels_h.to(dev), idx_h.to(dev) if with_idx else None, dl.t, rows.t, gscale)
    torch.cuda.synchronize()
    what = f"xent_rows B={B} CH={CH} idx={with_idx}"
    lab = labels_h[idx_h.long()] if with_idx else labels_h[:B]
    p64, b64 = part_h.double(), bias_h.double()
    x = torch.stack([sum(p64[k, s] for k, s in terms[b]) + b64 for b in range(B)])
    absum = torch.stack([sum(p64[k, s].abs() for k, s in terms[b]) + b64.abs() for b in range(B)])
    G = max(len(t) for t in terms) + 1
    if B > 1:
        assert x[B - 1, 2] == x[B - 1, 5] == x[B - 1].max()
    assert (x[0].max() - x[0].min()) >= 29.0
    rl, p = R.xent_rows64(x, lab)
    _, dref = R.xent64(x, lab, gscale)
    bd, bl = K.xent_rows_bounds(x, absum, G, lab, gscale, p, rl)
    ratio("xent_rows_dlogits", (B, CH, with_idx), dl.t, dref, bd, what)
    ratio("xent_rows_loss", (B, CH, with_idx), rows.t, rl, bl, what)
    dl.check(what)
    rows.check(what)


# ------------------------------------------------------------------------------------- sgd
SGD_SETS = {
    "plain": [dict()],  # (a momentum buffer is supplied and must keep its NaN fill)
    "momentum_first_then_next": [dict(momentum=0.9, first_step=True), dict(momentum=0.9)],
    "dampening": [dict(momentum=0.9, dampening=0.3)],
    "nesterov": [dict(momentum=0.9, nesterov=True)],
    "weight_decay": [dict(wd=1e-2), dict(wd=1e-2, momentum=0.8, dampening=0.1)],
    "maximize": [dict(maximize=True, momentum=0.5, wd=1e-3)],
    "shadow_only": [dict(update=False, momentum=0.9)],
    "no_mbuf": [dict(mbuf=False)],
}
SGD_N = [1, 3, 4, 5, 1023, 4 * 256 * 2048 + 7]


@pytest.mark.parametrize("name", list(SGD_SETS))
@pytest.mark.parametrize("n", SGD_N)
def test_sgd_per_element(C, n, name):
    """n = 4 * 256 * 2048 + 7 runs the grid-stride loop (2048 blocks x 256 threads x 4) and the
    3-element scalar tail.  A plain bf16 shadow over everything rides along."""
    lr = 0.05
    g0 = torch.Generator().manual_seed(200 + n % 97)
    p = Guarded((n,), F32)
    p.t.copy_(torch.randn(n, generator=g0))
    for step, kw in enumerate(SGD_SETS[name]):
        mom, damp, wd = kw.get("momentum", 0.0), kw.get("dampening", 0.0), kw.get("wd", 0.0)
        nest, maxi, first, upd = kw.get("nesterov", False), kw.get("maximize", False), kw.get("first_step", False), kw.get("update", True)
        grad = torch.randn(n, generator=g0).to(dev)
        if step == 0:
            mb = Guarded((n,), F32)
        if mom != 0.0 and not first and bool(torch.isnan(mb.t).any()):
            mb.t.copy_(torch.randn(n, generator=g0))  # a buffer from earlier steps
        p_in, m_in = p.t.clone(), mb.t.clone()
        sh = Guarded((n,), BF, fill=SENTINEL)
        C.sgd(p.t, grad, None if kw.get("mbuf") is False else mb.t, lr, mom, damp, wd, nest, maxi, first, upd,
              [(0, n, sh.t, K.SHADOW_BF16, 0, 0, 0)])
        torch.cuda.synchronize()
        what = f"sgd n={n} {name} step {step}"
        a = dict(lr=n32(lr), momentum=n32(mom), dampening=n32(damp), wd=n32(wd), nesterov=nest)
        if upd:
            pref, bref = R.sgd64(p_in, grad, m_in, maximize=maxi, first_step=first, **a)
            bp, bb = K.sgd_bounds(f64(p_in), f64(grad), f64(m_in) if mom != 0 and not first else f64(grad) * 0,
                                  first_step=first, **a)
            ratio("sgd_param_" + name, (n,), p.t, pref, bp, what)
            if mom != 0.0:
                ratio("sgd_momentum_" + name, (n,), mb.t, bref, bb, what)
            else:
                assert bool(torch.isnan(mb.t).all()), f"{what}: momentum 0 must leave the buffer alone"
            if n == 1023:  # torch's own optimizer in double
                tp = torch.nn.Parameter(f64(p_in).clone())
                opt = torch.optim.SGD([tp], lr=a["lr"], momentum=a["momentum"], dampening=a["dampening"],
                                      weight_decay=a["wd"], nesterov=nest, maximize=maxi)
                if mom != 0.0 and not first:
                    opt.state[tp]["momentum_buffer"] = f64(m_in).clone()
                tp.grad = f64(grad).clone()
                opt.step()
                torch.testing.assert_close(pref, tp.detach(), rtol=1e-13, atol=1e-15)
                ratio("sgd_vs_torch_" + name, (n,), p.t, tp.detach(), bp, what)
        else:
            assert torch.equal(bits(p.t), bits(p_in)) and torch.equal(bits(mb.t), bits(m_in)), f"{what}: shadow-only wrote"
        assert torch.equal(bits(sh.t), bits(p.t.to(BF))), f"{what}: shadow != bf16(stored parameter)"
        for g_ in (p, mb, sh):
            g_.check(what)


# (total n, [(off, n, kind, a, b, c)])
SHADOW_LAYOUTS = {
    "whole_aligned_all_kinds_a": (2048, [(0, 512, 1, 0, 0, 0), (512, 288, 2, 4, 9, 8), (1024, 512, 3, 16, 16, 0),
                                         (1536, 24, 4, 0, 0, 0)]),
    "whole_aligned_f32_kinds": (2048, [(0, 288, 5, 4, 9, 8), (512, 512, 6, 16, 16, 0)]),
    "off_unaligned": (1024, [(5, 512, 1, 0, 0, 0), (519, 288, 2, 4, 9, 8), (1, 288, 5, 4, 9, 8), (3, 21, 4, 0, 0, 0)]),
    "fcfrag_unaligned_off": (1030, [(6, 512, 3, 16, 16, 0), (518, 512, 6, 16, 16, 0)]),
    "n_not_multiple_of_4": (600, [(0, 27, 2, 3, 9, 1), (100, 27, 5, 3, 9, 1), (200, 33, 4, 0, 0, 0), (300, 101, 1, 0, 0, 0)]),
    "mid_quad_both_ends": (64, [(2, 9, 1, 0, 0, 0), (13, 6, 4, 0, 0, 0), (21, 27, 2, 3, 9, 1), (50, 1, 1, 0, 0, 0)]),
    "ends_in_scalar_tail": (1023, [(1000, 22, 1, 0, 0, 0), (993, 30, 4, 0, 0, 0), (996, 27, 5, 3, 9, 1), (1021, 2, 1, 0, 0, 0)]),
    "two_kinds_same_params": (18432 + 8, [(4, 18432, 1, 0, 0, 0), (4, 18432, 2, 64, 9, 32)]),
    "two_kinds_same_params_f32": (512, [(0, 512, 3, 16, 16, 0), (0, 512, 6, 16, 16, 0), (0, 512, 1, 0, 0, 0)]),
}


@pytest.mark.parametrize("update", [True, False])
@pytest.mark.parametrize("layout", list(SHADOW_LAYOUTS))
def test_sgd_shadows(C, layout, update):
    """Every shadow kind, whole and ragged regions: each written element is, bit for bit, the
    bf16 round-to-nearest-even (fp32 kinds: the copy) of the parameter this launch stored, at
    the index the kind defines; every other element keeps its sentinel (PAD4's 4th channel too)."""
    n, regions = SHADOW_LAYOUTS[layout]
    g0 = torch.Generator().manual_seed(7)
    p = Guarded((n,), F32)
    p.t.copy_(torch.randn(n, generator=g0))
    grad = torch.randn(n, generator=g0).to(dev)
    dsts = [Guarded((K.shadow_dst_numel(kind, rn),), F32 if K.shadow_is_f32(kind) else BF, fill=SENTINEL)
            for _, rn, kind, *_ in regions]
    C.sgd(p.t, grad, None, 0.1, 0.0, 0.0, 0.0, False, False, False, update,
          [(off, rn, d.t, kind, a, b, c) for (off, rn, kind, a, b, c), d in zip(regions, dsts)])
    torch.cuda.synchronize()
    stored = p.t.cpu()
    for (off, rn, kind, a, b, c), d in zip(regions, dsts):
        what = f"sgd shadow {layout} kind={kind} off={off} n={rn} update={update}"
        dt = F32 if K.shadow_is_f32(kind) else BF
        want = torch.full((K.shadow_dst_numel(kind, rn),), SENTINEL, dtype=dt)
        ix = torch.from_numpy(K.shadow_index(kind, rn, a, b, c))
        assert ix.unique().numel() == rn and int(ix.max()) < want.numel()
        want[ix] = stored[off:off + rn].to(dt)
        assert torch.equal(bits(d.t), bits(want)), what
        d.check(what)
    p.check(layout)


def test_sgd_shadow_binding_checks(C):
    p = torch.zeros(64, device=dev)
    for bad in ([(0, 27, torch.zeros(27, dtype=BF, device=dev), 2, 3, 9, 2)],       # Co*T*Ci != n
                [(0, 27, torch.zeros(27, dtype=BF, device=dev), 5, 3, 9, 1)],       # fp32 kind, bf16 dst
                [(0, 32, torch.zeros(32, device=dev), 6, 16, 8, 0)],                # C % 16
                [(60, 8, torch.zeros(8, dtype=BF, device=dev), 1, 0, 0, 0)],        # past the parameters
                [(0, 8, torch.zeros(8, dtype=BF, device=dev), 7, 0, 0, 0)]):        # unknown kind
        with pytest.raises(RuntimeError):
            C.sgd(p, p.clone(), None, 0.1, 0.0, 0.0, 0.0, False, False, False, True, bad)


# ----------------------------------------------------------------------- grad_reduce / scale_copy
RED_ROWS = [1, 2, 7, 16, 17, 28, 29, 33, 63, 64, 65, 112, 113, 129, 300]
RED_N = [1, 4, 63, 64, 65, 130]


def check_segment(out, rows32, GR, scale, prior, what, family, shape):
    """Both assertions for one reduced segment: the float64 bound and the order replay."""
    r64 = torch.from_numpy(rows32).double()
    ref = n32(scale) * r64.sum(0)
    p64 = None
    if prior is not None:
        p64 = torch.from_numpy(prior).double()
        ref = ref + p64
    r = ratio(family, shape, out, ref, K.reduce_bound(r64, n32(scale), p64), what)
    got = out.detach().cpu().numpy().view(np.int32)
    want = K.replay_finish(K.replay_reduce(rows32, GR), scale, prior)
    assert np.array_equal(got, want.view(np.int32)), f"{what}: differs from the order replay"
    return r


@pytest.mark.parametrize("rows", RED_ROWS)
def test_grad_reduce_single_segment(C, rows):
    """rows cross the first-batch condition (r + 7 GR < rows: 28/29 at GR = 4, 112/113 at 16), the
    64-row switch to 16 groups and the 16-row gate of the rows kernel; aligned calls with
    rows <= 16 take the rows kernel, every other the general one."""
    g0 = torch.Generator().manual_seed(300 + rows)
    GR = K.reduce_groups([rows])
    worst = 0.0
    for n in RED_N:
        for off, stride in ((0, (n + 3) // 4 * 4 + 4), (3, n + 8), (0, n), (4, n + 4 + 5)):
            for scale in (1.0, 1.0 / 3.0):
                for accum in (False, True):
                    slab = Guarded((rows, stride), F32)
                    slab.t.copy_(torch.randn(rows, stride, generator=g0))
                    dst = Guarded((n,), F32)
                    prior = None
                    if accum:
                        prior = torch.randn(n, generator=g0).numpy()
                        dst.t.copy_(torch.from_numpy(prior))
                    C.grad_reduce([(slab.t, stride, off, n, rows, dst.t, scale, accum)])
                    torch.cuda.synchronize()
                    what = f"grad_reduce rows={rows} n={n} off={off} stride={stride} scale={scale:.3f} accum={accum}"
                    rows32 = slab.t[:, off:off + n].cpu().numpy()
                    worst = max(worst, check_segment(dst.t, rows32, GR, scale, prior, what, "grad_reduce", (rows, n)))
                    dst.check(what)
                    slab.check(what)
    report_ratio(worst, "grad_reduce_rows_max", (rows,), tag="KERN_RATIO")


@pytest.mark.parametrize("nseg", [1, 2, 6])
def test_grad_reduce_segments(C, nseg):
    """One, two and six segments in one call: different rows, n, offsets, scales and accum per
    segment; the deepest segment (300 rows at six) selects 16 groups for all of them."""
    spec = [(7, 130, 3, 1.0, False), (33, 63, 0, 1.0 / 3.0, True), (300, 65, 1, 1.0, False), (1, 1, 0, 0.5, True),
            (16, 64, 4, 1.0, True), (65, 4, 2, 1.0 / 3.0, False)][:nseg]
    GR = K.reduce_groups([s[0] for s in spec])
    g0 = torch.Generator().manual_seed(310 + nseg)
    segs, keep = [], []
    for rows, n, off, scale, accum in spec:
        stride = n + off + 7
        slab, dst = Guarded((rows, stride), F32), Guarded((n,), F32)
        slab.t.copy_(torch.randn(rows, stride, generator=g0))
        prior = torch.randn(n, generator=g0).numpy() if accum else None
        if accum:
            dst.t.copy_(torch.from_numpy(prior))
        segs.append((slab.t, stride, off, n, rows, dst.t, scale, accum))
        keep.append((slab, dst, prior))
    C.grad_reduce(segs)
    torch.cuda.synchronize()
    for (rows, n, off, scale, accum), (slab, dst, prior) in zip(spec, keep):
        what = f"grad_reduce {nseg} segments: rows={rows} n={n} off={off}"
        check_segment(dst.t, slab.t[:, off:off + n].cpu().numpy(), GR, scale, prior, what, f"grad_reduce_{nseg}seg", (rows, n))
        dst.check(what)
        slab.check(what)
    with pytest.raises(RuntimeError):
        C.grad_reduce(segs * 7)


@pytest.mark.parametrize("rows", [1, 2, 4, 5, 7, 16, 17, 64])
@pytest.mark.parametrize("n", [4, 64, 132])
def test_grad_reduce_aligned_equals_shifted(C, rows, n):
    """The same rows through an aligned single-segment call (rows <= 16: the rows kernel) and
    shifted to an unaligned src_off (the general kernel): the same bits."""
    g0 = torch.Generator().manual_seed(320 + rows + n)
    data = torch.randn(rows, n, generator=g0)
    a_slab, b_slab = Guarded((rows, n), F32), Guarded((rows, n + 5), F32)
    a_slab.t.copy_(data)
    b_slab.t[:, 1:1 + n].copy_(data)
    for scale, accum in ((1.0, False), (1.0 / 3.0, False), (1.0, True), (1.0 / 3.0, True)):
        a, b = Guarded((n,), F32), Guarded((n,), F32)
        if accum:
            prior = torch.randn(n, generator=g0)
            a.t.copy_(prior)
            b.t.copy_(prior)
        C.grad_reduce([(a_slab.t, n, 0, n, rows, a.t, scale, accum)])
        C.grad_reduce([(b_slab.t, n + 5, 1, n, rows, b.t, scale, accum)])
        torch.cuda.synchronize()
        assert torch.equal(bits(a.t), bits(b.t)), f"rows={rows} n={n} scale={scale} accum={accum}: aligned != shifted"
        a.check()
        b.check()


@pytest.mark.parametrize("n", [1, 255, 256 * 1024 + 3])
def test_scale_copy(C, n):
    """One fp32 multiplication per element: the correctly rounded product, bit for bit."""
    g0 = torch.Generator().manual_seed(330)
    src = torch.randn(n, generator=g0)
    for scale in (1.0, 1.0 / 3.0, -0.37):
        dst = Guarded((n,), F32)
        C.scale_copy(dst.t, src.to(dev), scale)
        torch.cuda.synchronize()
        want = (src.numpy() * np.float32(scale)).astype(np.float32)
        assert np.array_equal(dst.t.cpu().numpy().view(np.int32), want.view(np.int32)), f"scale_copy n={n} scale={scale}"
        ref = src.double() * n32(scale)
        ratio("scale_copy", (n,), dst.t, ref, U * ref.abs() + 1e-45, f"scale_copy n={n}")
        dst.check(f"scale_copy n={n}")
