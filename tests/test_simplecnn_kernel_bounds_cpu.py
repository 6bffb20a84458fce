"""CPU side of tests/test_simplecnn_kernels_elementwise_gpu.py (no GPU needed).

1. The float64 references of ddp_amd/ops/reference.py that the GPU file measures the kernels
   against agree with torch's own double-precision operators.
2. The a-priori bounds of ddp_amd/ops/kernel_bounds.py admit a correct kernel: a float32
   emulation of each operation (torch's float32 operators - fp32 accumulation in another order
   than the float64 reference - with a bf16 rounding of the output where the kernel rounds)
   stays inside the bound on the inputs the GPU file uses.  Evidence about the inputs and the
   bounds, not about the kernels.
3. The bounds reject a subtly wrong kernel: from that emulated output, one border element
   moved by 3 bf16 ulps (fp32 outputs: 16 fp32 ulps of the accumulated magnitude), one tap
   dropped at one image-edge pixel, the bias omitted for one channel, one slab row skipped in a
   reduction and one shadow element written at the neighbouring index each fail; for conv1,
   fc, the fused-fc partials, xent_rows and scale_copy the matching wrong outputs (a missing
   bias, tap, pixel, row, partial or the / 255 left out).
4. The reduction-order replay is self-consistent.

The moved-element case is asserted where the arithmetic lets a bound see it: bf16 outputs
(3 bf16 ulps against 2**-8 |ref|) and short fp32 chains (SGD: 16 ulps against 6 u P; the fc
weight gradient: at most 15 u A).  The
worst-case bound of an n-term fp32 accumulation, 2 n u A, admits n ulps of A by construction
(289 terms for conv2, 224 pixel slots for a slab row), so 16 ulps cannot leave it; the fp32
conv outputs are held by the dropped-tap, omitted-bias and skipped-row cases instead.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise
from ddp_amd.ops import kernel_bounds as K
from ddp_amd.ops import reference as R
from ddp_amd.ops.kernel_bounds import U, acc_bound, bf16_store_bound, ratio, ratio_value

BF = torch.bfloat16
SHAPES = [(1, 28, 28, 32, 64), (3, 28, 28, 32, 64), (2, 5, 7, 32, 64), (2, 6, 12, 32, 128), (2, 6, 12, 64, 64), (2, 6, 12, 64, 128), (2, 4, 40, 32, 64), (2, 12, 12, 32, 64)]
DTS = [pytest.param(BF, id="bf16"), pytest.param(torch.float32, id="fp32")]
rnd = functools.partial(elementwise.rnd, device="cpu")


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_inputs(B, H, W, Cin, Cout, dtype, seed=100):
    return (rnd(B, H, W, Cin, relu=True, seed=seed, dtype=dtype), rnd(Cout, 3, 3, Cin, scale=0.1, seed=seed + 1, dtype=dtype),
            rnd(Cout, scale=0.1, seed=seed + 2, dtype=torch.float32))


def close64(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- 1. the references
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_conv_references_match_torch_double(B, H, W, Cin, Cout):
    x, w, b = (t.double() for t in conv_inputs(B, H, W, Cin, Cout, BF))
    xt = nchw(x).clone().requires_grad_(True)
    wt = w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xt, wt, b, padding=1)
    close64(R.conv3x3_64(x, w, b), nhwc(y.detach()))
    close64(R.conv3x3_64(x, w, b, relu=True), nhwc(torch.relu(y.detach())))
    dy = rnd(B, H, W, Cout, scale=0.5, seed=7).double()
    y.backward(nchw(dy))
    close64(R.conv3x3_dgrad64(dy, w), nhwc(xt.grad))
    dw, db = R.conv3x3_wgrad64(dy, x)
    close64(dw, wt.grad.permute(0, 2, 3, 1))
    close64(db, dy.sum(dim=(0, 1, 2)))
    # row chunks of single images add up to the whole gradient
    Rr = 5 if H > 5 else 2
    parts = [R.conv3x3_wgrad64(dy, x, rows=(r0, min(H, r0 + Rr)), image=n) for n in range(B) for r0 in range(0, H, Rr)]
    close64(sum(p[0] for p in parts), dw)
    close64(sum(p[1] for p in parts), db)


@pytest.mark.parametrize("B", [1, 3])
def test_conv1_fc_xent_sgd_references_match_torch_double(B):
    H = W = 28
    g0 = torch.Generator().manual_seed(1)
    x8 = torch.randint(0, 256, (B, H, W), generator=g0, dtype=torch.uint8)
    w1, b1 = torch.randn(32, 9, generator=g0).double(), torch.randn(32, generator=g0).double()
    xd = (x8.double() / 255.0).unsqueeze(1).requires_grad_(False)
    w1t = w1.reshape(32, 1, 3, 3).clone().requires_grad_(True)
    y = F.conv2d(xd, w1t, b1, padding=1)
    close64(R.conv1_64(x8, w1, b1), nhwc(torch.relu(y.detach())))
    dz = rnd(B, H, W, 32, seed=2).double()
    y.backward(nchw(dz))
    dw, db = R.conv1_wgrad64(dz, x8)
    close64(dw, w1t.grad.reshape(32, 9))
    close64(db, dz.sum(dim=(0, 1, 2)))
    chunks = [R.conv1_wgrad64(dz, x8, (p0, min(p0 + 256, B * 784))) for p0 in range(0, B * 784, 256)]
    close64(sum(c[0] for c in chunks), dw)
    # fc and its backward
    a = rnd(B, H, W, 64, relu=True, seed=3).double().requires_grad_(True)
    wf = rnd(10, 784, 64, scale=0.05, seed=4).double().requires_grad_(True)
    bf = torch.randn(10, generator=g0).double()
    out = F.linear(a.reshape(B, -1), wf.reshape(10, -1), bf)
    close64(R.fc64(a, wf, bf), out.detach())
    dl = torch.randn(B, 10, generator=g0).double()
    out.backward(dl)
    dx, dwf, dbf = R.fc_bwd64(dl, a, wf, 0.37, mask=False)
    close64(dx, a.grad)
    close64(dwf, 0.37 * wf.grad)
    close64(dbf, 0.37 * dl.sum(0))
    close64(R.fc_bwd64(dl, a, wf, 1.0, mask=True)[0], a.grad * (a.detach() > 0))
    # block partials fold to the logits, for blocks inside an image and straddling two
    for CH in (64, 128):
        part = R.fc_block_partials64(a, wf, CH)
        fold = torch.zeros(B, 10, dtype=torch.float64)
        for k in range(part.shape[0]):
            n0 = k * CH // 784
            fold[n0] += part[k, 0]
            if n0 + 1 < B:
                fold[n0 + 1] += part[k, 1]
            else:
                assert bool((part[k, 1] == 0).all())
        close64(fold, R.fc64(a, wf))
    # cross-entropy
    lab = torch.randint(0, 10, (B,), generator=g0)
    lg = out.detach().clone().requires_grad_(True)
    loss = F.cross_entropy(lg, lab)
    loss.backward()
    rl, dref = R.xent64(lg.detach(), lab)
    close64(rl, loss.detach())
    close64(dref, lg.grad)
    # SGD
    n = 257
    for kw in (dict(), dict(momentum=0.9), dict(momentum=0.9, dampening=0.3), dict(momentum=0.9, nesterov=True),
               dict(weight_decay=1e-2, momentum=0.5), dict(maximize=True, momentum=0.5)):
        p0, g1, g2 = (torch.randn(n, generator=g0).double() for _ in range(3))
        tp = torch.nn.Parameter(p0.clone())
        opt = torch.optim.SGD([tp], lr=0.05, **kw)
        a_ = dict(lr=0.05, momentum=kw.get("momentum", 0.0), dampening=kw.get("dampening", 0.0),
                  wd=kw.get("weight_decay", 0.0), nesterov=kw.get("nesterov", False), maximize=kw.get("maximize", False))
        p, m = p0, None
        for step, g in enumerate((g1, g2)):
            tp.grad = g.clone()
            opt.step()
            p, m = R.sgd64(p, g, m, first_step=step == 0, **a_)
            close64(p, tp.detach())


# ------------------------------------------------- 2. + 3. admit a correct kernel, reject a wrong one
def emulate(t32, dtype):
    """The float32 result as the kernel stores it."""
    return t32.to(BF) if dtype == BF else t32


def bump(out, i, ulps_bf16=3, A=None):
    """out with element i moved by 3 bf16 ulps (bf16) or 16 fp32 ulps of the magnitude A (fp32)."""
    o = out.clone()
    if out.dtype == BF:
        v = o[i].float().abs().clamp(min=2.0 ** -126)
        o[i] = (o[i].float() + ulps_bf16 * 2.0 ** (torch.floor(torch.log2(v)) - 7)).to(BF)
    else:
        mag = torch.as_tensor(A, dtype=torch.float64).clamp(min=2.0 ** -126)
        o[i] = (o[i].double() + 16 * 2.0 ** (torch.floor(torch.log2(mag)) - 23)).float()
    return o


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_conv_fwd_bound_admits_and_rejects(B, H, W, Cin, Cout, dtype):
    x, w, b = conv_inputs(B, H, W, Cin, Cout, dtype)
    f32 = dtype == torch.float32
    ref = R.conv3x3_64(x, w, b, True)
    A = R.conv3x3_64(x.abs(), w.abs(), b.abs())
    E = acc_bound(9 * Cin + 1, A, f32)
    bound = bf16_store_bound(ref, E) if dtype == BF else E
    y32 = nhwc(torch.relu(F.conv2d(nchw(x.float()), w.float().permute(0, 3, 1, 2), b, padding=1)))
    out = emulate(y32, dtype)
    ratio("cpu_fwd", (B, H, W, Cin, Cout), out, ref, bound, "float32 emulation", tag="CPU_RATIO")
    # a border element that is not clamped by the ReLU, moved
    pos = torch.nonzero(ref[0, 0] > 0.05)[0]
    i = (0, 0, int(pos[0]), int(pos[1]))
    if dtype == BF:  # (fp32: see the module docstring - an n-term worst-case bound admits n ulps)
        assert ratio_value(bump(out, i, A=A[i]), ref, bound) > 1.0
    # one tap dropped at that image-edge pixel: the centre tap of its largest contribution
    drop = R.conv3x3_64(x, w, b, False)
    drop[0, 0, int(pos[0])] -= w.double()[:, 1, 1, :] @ x.double()[0, 0, int(pos[0])]
    drop = torch.relu(drop)
    assert (drop - ref).abs().max() > 0 and ratio_value(emulate(drop.float(), dtype), ref, bound) > 1.0
    # the bias omitted for one channel
    nb = b.clone()
    nb[int(pos[1])] = 0.0
    no_bias = nhwc(torch.relu(F.conv2d(nchw(x.float()), w.float().permute(0, 3, 1, 2), nb, padding=1)))
    assert ratio_value(emulate(no_bias, dtype), ref, bound) > 1.0


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_conv_dgrad_wgrad_bounds_admit_and_reject(B, H, W, Cin, Cout, dtype):
    f32 = dtype == torch.float32
    dy = rnd(B, H, W, Cout, scale=0.5, seed=120, dtype=dtype)
    xact = rnd(B, H, W, Cin, seed=122, relu=True, dtype=dtype)
    w = rnd(Cout, 3, 3, Cin, scale=0.1, seed=123, dtype=dtype)
    keep = xact.double() > 0
    ref = R.conv3x3_dgrad64(dy, w) * keep
    A = R.conv3x3_dgrad64(dy.abs(), w.abs()) * keep
    E = acc_bound(9 * Cout, A, f32)
    bound = bf16_store_bound(ref, E) if dtype == BF else E
    d32 = nhwc(F.conv_transpose2d(nchw(dy.float()), w.float().permute(0, 3, 1, 2), padding=1)) * keep
    out = emulate(d32, dtype)
    ratio("cpu_dgrad", (B, H, W, Cin, Cout), out, ref, bound, "float32 emulation", tag="CPU_RATIO")
    pos = torch.nonzero(keep[0, 0] & (ref[0, 0].abs() > 0.05))[0]
    i = (0, 0, int(pos[0]), int(pos[1]))
    if dtype == BF:
        assert ratio_value(bump(out, i, A=A[i]), ref, bound) > 1.0
    # a masked element that is not exactly 0 has no slack at all
    j = tuple(int(v) for v in torch.nonzero(~keep)[0])
    leak = out.clone()
    leak[j] = 2.0 ** -20
    assert ratio_value(leak, ref, bound) > 1.0
    # weight gradient: the whole-image slab row and the reduction over images
    x = rnd(B, H, W, Cin, seed=142, relu=True, dtype=dtype)
    Wp = (W + 7) & ~7
    nslot = (H * Wp + 31) // 32 * 32
    rows_ref, rows_A, rows32 = [], [], []
    for n in range(B):
        dw, db = R.conv3x3_wgrad64(dy, x, image=n)
        aw, ab = R.conv3x3_wgrad64(dy.abs(), x.abs(), image=n)
        rows_ref.append(torch.cat([dw.reshape(-1), db])); rows_A.append(torch.cat([aw.reshape(-1), ab]))
        g32 = torch.nn.grad.conv2d_weight(nchw(x[n:n + 1].float()), (Cout, Cin, 3, 3), nchw(dy[n:n + 1].float()), padding=1)
        rows32.append(torch.cat([g32.permute(0, 2, 3, 1).reshape(-1), dy[n].float().sum(dim=(0, 1))]))
    rows_ref, rows_A, rows32 = torch.stack(rows_ref), torch.stack(rows_A), torch.stack(rows32)
    Ew = acc_bound(nslot, rows_A, f32)
    ratio("cpu_wgrad_slab", (B, H, W, Cin, Cout), rows32, rows_ref, Ew, "float32 emulation", tag="CPU_RATIO")
    # (a slab element moved by 16 ulps stays inside 2 n u A at n = nslot >= 32 terms: the slabs are
    # guarded by the skipped-row case below and by the GPU file's bitwise reducer replay)
    if B > 1:  # one slab row skipped by the reducer
        tot = Ew.sum(0) + K.reduce_bound(rows32.double(), 1.0)
        red = torch.from_numpy(K.replay_reduce(rows32.numpy(), 4))
        ratio("cpu_wgrad_reduced", (B, H, W, Cin, Cout), red, rows_ref.sum(0), tot, "replay", tag="CPU_RATIO")
        skipped = torch.from_numpy(K.replay_reduce(rows32[:-1].numpy(), 4))
        assert ratio_value(skipped, rows_ref.sum(0), tot) > 1.0


@pytest.mark.parametrize("rows", [1, 2, 7, 16, 17, 28, 29, 33, 63, 64, 65, 112, 113, 129, 300])
def test_reduce_bound_admits_replay_and_rejects_a_skipped_row(rows):
    g0 = torch.Generator().manual_seed(rows)
    GR = K.reduce_groups([rows])
    for n in (1, 4, 63, 64, 65, 130):
        for scale in (1.0, 1.0 / 3.0):
            slab = torch.randn(rows, n, generator=g0)
            prior = torch.randn(n, generator=g0)
            s32 = float(np.float32(scale))
            ref = s32 * slab.double().sum(0) + prior.double()
            bound = K.reduce_bound(slab.double(), s32, prior.double())
            cand = K.replay_finish(K.replay_reduce(slab.numpy(), GR), scale, prior.numpy())
            ratio("cpu_reduce", (rows, n), torch.from_numpy(cand), ref, bound, "replay", tag="CPU_RATIO")
            if rows > 1:
                r = int(slab.abs().sum(1).argmax())
                cut = torch.cat([slab[:r], slab[r + 1:]])
                bad = K.replay_finish(K.replay_reduce(cut.numpy(), GR), scale, prior.numpy())
                assert ratio_value(torch.from_numpy(bad), ref, bound) > 1.0


@pytest.mark.parametrize("kw", [dict(), dict(momentum=0.9, first_step=True), dict(momentum=0.9),
                                dict(momentum=0.9, dampening=0.3), dict(momentum=0.9, nesterov=True), dict(wd=1e-2),
                                dict(wd=1e-2, momentum=0.8, dampening=0.1)], ids=str)
def test_sgd_bound_admits_float32_and_rejects_16_ulps(kw):
    n = 4099
    g0 = torch.Generator().manual_seed(5)
    p, g, m = (torch.randn(n, generator=g0) for _ in range(3))
    first = kw.pop("first_step", False)
    a = dict(lr=float(np.float32(0.05)), momentum=float(np.float32(kw.get("momentum", 0.0))),
             dampening=float(np.float32(kw.get("dampening", 0.0))), wd=float(np.float32(kw.get("wd", 0.0))),
             nesterov=kw.get("nesterov", False))
    pref, bref = R.sgd64(p, g, m, first_step=first, **a)
    bp, bb = K.sgd_bounds(p.double(), g.double(), m.double() if not first else m.double() * 0, first_step=first, **a)
    # float32, torch's own sequence of operations (another order of roundings than the fma chain)
    d = g + np.float32(a["wd"]) * p if a["wd"] else g.clone()
    buf = None
    if a["momentum"]:
        buf = d.clone() if first else m * np.float32(a["momentum"]) + d * np.float32(1.0 - a["dampening"])
        d = d + buf * np.float32(a["momentum"]) if a["nesterov"] else buf
    out = p - d * np.float32(a["lr"])
    ratio("cpu_sgd_param", (n,), out, pref, bp, "float32 emulation", tag="CPU_RATIO")
    if buf is not None:
        ratio("cpu_sgd_momentum", (n,), buf, bref, bb, "float32 emulation", tag="CPU_RATIO")
    i = int(p.abs().argmax())
    assert ratio_value(bump(out, (i,), A=p[i].abs()), pref, bp) > 1.0


@pytest.mark.parametrize("kind,n,a,b,c", [(1, 37, 0, 0, 0), (2, 288, 4, 9, 8), (3, 512, 16, 16, 0), (4, 21, 0, 0, 0),
                                          (5, 27, 3, 9, 1), (6, 512, 16, 16, 0)])
def test_shadow_index_is_a_layout_and_a_neighbour_write_is_caught(kind, n, a, b, c):
    ix = K.shadow_index(kind, n, a, b, c)
    m = K.shadow_dst_numel(kind, n)
    assert len(np.unique(ix)) == n and ix.min() >= 0 and ix.max() < m
    g0 = torch.Generator().manual_seed(kind)
    p = torch.randn(n, generator=g0)
    dt = torch.float32 if K.shadow_is_f32(kind) else BF
    want = torch.full((m,), 1152.0, dtype=dt)
    want[torch.from_numpy(ix)] = p.to(dt)
    # the layouts against their definitions
    if kind in (2, 5):
        assert torch.equal(want, p.view(a, b, c).permute(1, 2, 0).reshape(-1).to(dt))
    if kind in (3, 6):
        from ddp_amd.ops.functional import fc_weight_frag
        assert torch.equal(want, fc_weight_frag(p, a, b, dt).reshape(-1))
    if kind == 4:
        v = want.view(-1, 4)
        assert torch.equal(v[:, :3].reshape(-1), p.to(dt)) and bool((v[:, 3] == 1152.0).all())
    # one element written at the neighbouring index instead: the bit comparison sees it
    j = n // 2
    wrong = torch.full((m,), 1152.0, dtype=dt)
    ix2 = ix.copy()
    ix2[j] = ix[j] + 1 if ix[j] + 1 < m else ix[j] - 1
    wrong[torch.from_numpy(ix2)] = p.to(dt)
    assert not torch.equal(wrong.view(torch.int16 if dt == BF else torch.int32),
                           want.view(torch.int16 if dt == BF else torch.int32))


# ------------------------------------------- conv1, fc, fused-fc partials, xent_rows, scale_copy
@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("B", [1, 3])
def test_conv1_bounds_admit_and_reject(B, dtype):
    H = W = 28
    f32 = dtype == torch.float32
    g0 = torch.Generator().manual_seed(150)
    w, b = torch.randn(32, 9, generator=g0) * 0.3, torch.randn(32, generator=g0) * 0.1
    xf = torch.rand(B, H, W, generator=g0)
    x8 = torch.randint(0, 256, (B, H, W), generator=g0, dtype=torch.uint8)
    w4 = w.reshape(32, 1, 3, 3)
    for name, xin, nterm in (("float", xf, 10), ("u8", x8, 11)):
        x32 = xin.float() / np.float32(255.0) if name == "u8" else xin
        xa = xin.double() / 255.0 if name == "u8" else xin.double()
        ref = R.conv1_64(xin, w, b)
        A = R.conv3x3_64(xa.unsqueeze(-1), w.double().abs().reshape(32, 3, 3, 1), b.double().abs())
        E = acc_bound(nterm, A)
        bound = bf16_store_bound(ref, E) if dtype == BF else E
        out = emulate(nhwc(torch.relu(F.conv2d(x32.unsqueeze(1), w4, b, padding=1))), dtype)
        ratio(f"cpu_conv1_fwd_{name}", (B,), out, ref, bound, "float32 emulation", tag="CPU_RATIO")
        pos = torch.nonzero(ref[0, 0] > 0.2)[0]
        i = (0, 0, int(pos[0]), int(pos[1]))
        if dtype == BF:  # (fp32: 16 ulps of A lie between 16 u A and 32 u A, astride the bound 20 u A)
            assert ratio_value(bump(out, i, A=A[i]), ref, bound) > 1.0
        nb = b.clone()
        nb[int(pos[1])] = 0.0
        assert ratio_value(emulate(nhwc(torch.relu(F.conv2d(x32.unsqueeze(1), w4, nb, padding=1))), dtype), ref, bound) > 1.0
        if name == "u8":  # the / 255 left out
            raw = emulate(nhwc(torch.relu(F.conv2d(xin.float().unsqueeze(1), w4, b, padding=1))), dtype)
            assert ratio_value(raw, ref, bound) > 1.0
        # weight gradient slab rows
        dz = (rnd(B, H, W, 32, scale=0.5, seed=161, dtype=dtype).double()
              * (rnd(B, H, W, 32, seed=162, relu=True, dtype=dtype).double() > 0))
        for chunk in (196, 256):
            refs, As, outs = [], [], []
            for p0 in range(0, B * H * W, chunk):
                px = (p0, min(p0 + chunk, B * H * W))
                dw, db = R.conv1_wgrad64(dz, xin, px)
                aw, ab = R.conv1_wgrad64(dz.abs(), xin, px)
                refs.append(torch.cat([dw.reshape(-1), db])); As.append(torch.cat([aw.reshape(-1), ab]))
                keep = torch.zeros(B * H * W)
                keep[px[0]:px[1]] = 1.0
                d32 = dz.float() * keep.view(B, H, W, 1)
                g32 = torch.nn.grad.conv2d_weight(x32.unsqueeze(1), (32, 1, 3, 3), nchw(d32), padding=1)
                outs.append(torch.cat([g32.reshape(-1), d32.sum(dim=(0, 1, 2))]))
            refs, As, outs = torch.stack(refs), torch.stack(As), torch.stack(outs)
            Ew = acc_bound(chunk + (1 if name == "u8" else 0), As, f32)
            ratio(f"cpu_conv1_wgrad_{name}", (B, chunk), outs, refs, Ew, "float32 emulation", tag="CPU_RATIO")
            # one pixel of the block left out of one channel's sums
            k = int(As[0, :288].argmax())
            co = k // 9
            pmax = int(dz.reshape(-1, 32)[:min(chunk, B * H * W), co].abs().argmax())
            cut = dz.clone()
            cut.view(-1, 32)[pmax, co] = 0.0
            bad = outs.clone()
            dwc, dbc = R.conv1_wgrad64(cut, xin, (0, min(chunk, B * H * W)))
            bad[0] = torch.cat([dwc.reshape(-1), dbc]).float()
            assert ratio_value(bad, refs, Ew) > 1.0


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("B", [1, 3])
def test_fc_bounds_admit_and_reject(B, dtype):
    H = W = 28
    HW, Cc, NO, scale = H * W, 64, 10, float(np.float32(0.37))
    f32 = dtype == torch.float32
    x = rnd(B, H, W, Cc, relu=True, seed=170, dtype=dtype)
    wfc = rnd(NO, HW, Cc, scale=0.05, seed=171, dtype=dtype)
    bfc = rnd(NO, scale=0.1, seed=172, dtype=torch.float32)
    x2, w2 = x.float().reshape(B, -1), wfc.float().reshape(NO, -1)
    # fc_partial (per 16-pixel tile) and fc_reduce
    xt, wt = x.double().reshape(B, HW // 16, 16 * Cc), wfc.double().reshape(NO, HW // 16, 16 * Cc)
    pref, pA = torch.einsum("bgk,ogk->bgo", xt, wt), torch.einsum("bgk,ogk->bgo", xt.abs(), wt.abs())
    p32 = torch.einsum("bgk,ogk->bgo", xt.float(), wt.float())
    Ep = acc_bound(16 * Cc + 6, pA, f32)
    ratio("cpu_fc_partial", (B,), p32, pref, Ep, "float32 emulation", tag="CPU_RATIO")
    miss = torch.einsum("bgk,ogk->bgo", xt.float()[:, :, 64:], wt.float()[:, :, 64:])  # one pixel of a tile left out
    assert ratio_value(miss, pref, Ep) > 1.0
    # fc_reduce: from the partials it reads (G sequential adds and the bias)
    ref = p32.double().sum(1) + bfc.double()
    Eo = acc_bound(HW // 16 + 1, p32.double().abs().sum(1) + bfc.double().abs())
    ratio("cpu_fc_reduce", (B,), p32.sum(1) + bfc, ref, Eo, "float32 emulation", tag="CPU_RATIO")
    assert ratio_value(p32.sum(1), ref, Eo) > 1.0                           # the bias omitted
    assert ratio_value(p32[:, 1:].sum(1) + bfc, ref, Eo) > 1.0              # one tile's partial skipped
    # the fused epilogue's block partials, from a stored activation
    for CH in (64, 128):
        bref = R.fc_block_partials64(x, wfc, CH)
        bA = R.fc_block_partials64(x.abs(), wfc.abs(), CH)
        Eb = acc_bound(64 * CH + CH // 4, bA, f32)
        b32 = torch.zeros_like(bref, dtype=torch.float32)
        xf_, wf_ = x.float().reshape(B * HW, Cc), wfc.float()
        for k in range(bref.shape[0]):
            p0, p1 = k * CH, min((k + 1) * CH, B * HW)
            n0 = p0 // HW
            for slot in (0, 1):
                a_, b_ = max(p0, (n0 + slot) * HW), min(p1, (n0 + slot + 1) * HW)
                if a_ < b_:
                    b32[k, slot] = torch.einsum("pc,opc->o", xf_[a_:b_], wf_[:, a_ - (n0 + slot) * HW:b_ - (n0 + slot) * HW])
        ratio("cpu_fc_block_partials", (B, CH), b32, bref, Eb, "float32 emulation", tag="CPU_RATIO")
        bad = b32.clone()  # one 16-pixel tile of block 0 dropped
        bad[0, 0] -= torch.einsum("pc,opc->o", xf_[:16], wf_[:, :16])
        assert ratio_value(bad, bref, Eb) > 1.0
        if B > 1:  # a straddling block's second image written into slot 0 as well
            ks = next(k for k in range(bref.shape[0]) if bool((bref[k, 1] != 0).any()))
            bad = b32.clone()
            bad[ks, 0] += b32[ks, 1]
            assert ratio_value(bad, bref, Eb) > 1.0
    # fc_bwd
    dl = rnd(B, NO, scale=0.1, seed=182, dtype=torch.float32)
    rows = rnd(B, seed=183, dtype=torch.float32).abs() + 0.5
    for mask in (True, False):
        rdx, rdw, rdb = R.fc_bwd64(dl, x, wfc, scale, mask)
        adx, adw, adb = R.fc_bwd64(dl.abs(), x, wfc.abs(), scale, mask)
        Edx = acc_bound(NO, adx, f32)
        bdx = bf16_store_bound(rdx, Edx) if dtype == BF else Edx
        dx32 = (dl @ w2) * ((x2 > 0) if mask else 1.0)
        odx = emulate(dx32.view_as(x), dtype)
        ratio("cpu_fc_bwd_dx", (B, mask), odx, rdx, bdx, "float32 emulation", tag="CPU_RATIO")
        i = tuple(int(v) for v in torch.nonzero((x.double() > 0) & (rdx.abs() > 1e-3))[0])
        if dtype == BF:  # (fp32: 10 terms, as conv1)
            assert ratio_value(bump(odx, i, A=adx[i]), rdx, bdx) > 1.0
        dx9 = (dl[:, :9] @ w2[:9]) * ((x2 > 0) if mask else 1.0)           # one class left out
        assert ratio_value(emulate(dx9.view_as(x), dtype), rdx, bdx) > 1.0
        Edw = acc_bound(B + 2, adw, f32)
        dw32 = ((dl.t() @ x2) * np.float32(scale)).view_as(wfc)
        ratio("cpu_fc_bwd_dw", (B, mask), dw32, rdw, Edw, "float32 emulation", tag="CPU_RATIO")
        assert ratio_value((dl.t() @ x2).view_as(wfc), rdw, Edw) > 1.0      # the scale omitted
        j = tuple(int(v) for v in torch.nonzero(adw == adw.max())[0])
        assert ratio_value(bump(dw32, j, A=adw[j]), rdw, Edw) > 1.0
        Edb = acc_bound(B + 2, adb)
        ratio("cpu_fc_bwd_dbias", (B, mask), dl.sum(0) * np.float32(scale), rdb, Edb, "float32 emulation", tag="CPU_RATIO")
        assert ratio_value(dl[1:].sum(0) * np.float32(scale) if B > 1 else dl.sum(0), rdb, Edb) > 1.0  # a row / the scale omitted
    lref = rows.double().mean().reshape(1)
    El = acc_bound(B + 1, rows.double().abs().mean().reshape(1))
    ratio("cpu_fc_bwd_loss", (B,), (rows.sum() / B).reshape(1), lref, El, "float32 emulation", tag="CPU_RATIO")
    assert ratio_value(rows.sum().reshape(1) / (B + 1), lref, El) > 1.0


def fold_terms(b, HW, CH):
    p0 = b * HW
    kb0, kb1 = p0 // CH, (p0 + HW - 1) // CH
    return [(kb0 + j, (0 if kb0 * CH == p0 else 1) if j == 0 else 0) for j in range(kb1 - kb0 + 1)]


@pytest.mark.parametrize("CH", [64, 128])
@pytest.mark.parametrize("B", [1, 3, 7])
def test_xent_rows_bound_admits_and_rejects(B, CH):
    """The GPU file's inputs (a row 30 apart, a row with tied maxima) through float32 torch
    operators; a partial left out of a logit, the bias left out, and a loss computed against
    the neighbouring label are rejected."""
    HW, NO = 784, 10
    nblk = -(-B * HW // CH)
    g0 = torch.Generator().manual_seed(190 + B)
    part = torch.randn(nblk, 2, NO, generator=g0) * 0.7
    bias = torch.randn(NO, generator=g0) * 0.1
    bias[5] = bias[2]
    terms = [fold_terms(b, HW, CH) for b in range(B)]
    k0, s0 = terms[0][0]
    part[k0, s0, 0] += 15.0
    part[k0, s0, 9] -= 15.0
    if B > 1:
        for k, s in terms[B - 1]:
            part[k, s] = 0.0
        k, s = terms[B - 1][0]
        part[k, s] = torch.tensor([0.25, -1.0, 1.5, 0.5, -0.75, 1.5, 0.0, -2.0, 1.0, 0.125])
    lab = torch.randint(0, NO, (B,), generator=g0)
    gscale = float(np.float32(1.0 / B))
    p64, b64 = part.double(), bias.double()
    x = torch.stack([sum(p64[k, s] for k, s in terms[b]) + b64 for b in range(B)])
    absum = torch.stack([sum(p64[k, s].abs() for k, s in terms[b]) + b64.abs() for b in range(B)])
    G = max(len(t) for t in terms) + 1
    rl, p = R.xent_rows64(x, lab)
    _, dref = R.xent64(x, lab, gscale)
    bd, bl = K.xent_rows_bounds(x, absum, G, lab, gscale, p, rl)

    def f32_eval(skip=None, with_bias=True, labels=lab):
        lg = torch.stack([sum((part[k, s] for k, s in terms[b] if (b, k) != skip), torch.zeros(NO)) for b in range(B)])
        lg = lg + bias if with_bias else lg
        lp = torch.log_softmax(lg, 1)
        d = lp.exp()
        d[torch.arange(B), labels] -= 1.0
        return d * np.float32(gscale), -lp[torch.arange(B), labels]

    d32, l32 = f32_eval()
    ratio("cpu_xent_rows_dlogits", (B, CH), d32, dref, bd, "float32 emulation", tag="CPU_RATIO")
    ratio("cpu_xent_rows_loss", (B, CH), l32, rl, bl, "float32 emulation", tag="CPU_RATIO")
    b_mid = B // 2 if B > 2 else 0
    d_bad, l_bad = f32_eval(skip=(b_mid, terms[b_mid][-1][0]))
    # (B = 1 is the saturated 30-apart row: its softmax does not move, its loss does)
    assert ratio_value(l_bad, rl, bl) > 1.0 and (B == 1 or ratio_value(d_bad, dref, bd) > 1.0)
    d_bad, l_bad = f32_eval(with_bias=False)
    assert ratio_value(l_bad, rl, bl) > 1.0 and (B == 1 or ratio_value(d_bad, dref, bd) > 1.0)
    d_bad, l_bad = f32_eval(labels=(lab + 1) % NO)
    assert ratio_value(d_bad, dref, bd) > 1.0
    # 16 fp32 ulps on one dlogit of probability about one half (the tied row): outside p (2 D + 64) u?
    # No - 64 u p admits it; the absolute term 2 u g is what a stray value at a p -> 0 class meets:
    r0 = int(p[0].argmin())
    stray = d32.clone()
    stray[0, r0] += np.float32(16 * 2.0 ** -23 * gscale)
    assert ratio_value(stray, dref, bd) > 1.0


@pytest.mark.parametrize("n", [1, 255, 256 * 1024 + 3])
def test_scale_copy_bound_admits_one_rounding_and_rejects_two_ulps(n):
    g0 = torch.Generator().manual_seed(330)
    src = torch.randn(n, generator=g0)
    for scale in (1.0 / 3.0, -0.37):
        s32 = float(np.float32(scale))
        ref = src.double() * s32
        bound = U * ref.abs() + 1e-45
        out = src * np.float32(scale)
        ratio("cpu_scale_copy", (n,), out, ref, bound, "float32 product", tag="CPU_RATIO")
        i = int(src.abs().argmax())
        bad = out.clone()
        bad[i] = torch.nextafter(torch.nextafter(bad[i], bad[i] * 2), bad[i] * 2)
        assert ratio_value(bad, ref, bound) > 1.0
        assert ratio_value(src * np.float32(scale) * np.float32(1.0 + 2.0 ** -22), ref, bound) > 1.0


# ------------------------------------------------------------------ 4. the order replay
def test_replay_is_sequential_for_few_rows_and_not_pairwise():
    """One row per group (rows <= GR) is plain sequential float32 addition: rows <= 16 at 16
    groups, rows <= 4 at 4 groups; more rows per group is a different order, and a pairwise
    tree another one still."""
    g0 = torch.Generator().manual_seed(11)
    for rows in range(1, 9):
        slab = torch.randn(rows, 257, generator=g0).numpy()
        seq = K.replay_sequential(slab)
        assert np.array_equal(K.replay_reduce(slab, 16).view(np.int32), seq.view(np.int32))
        if rows <= 4:
            assert np.array_equal(K.replay_reduce(slab, 4).view(np.int32), seq.view(np.int32))
        assert np.abs(seq.astype(np.float64) - slab.astype(np.float64).sum(0)).max() < 1e-5
    # 1 + u + u + u: sequentially every add is a tie that rounds back to 1; pairwise (1 + u) + (u + u)
    # = 1 + 2 u is exact
    u = np.float32(2.0 ** -24)
    col = np.array([[1.0], [u], [u], [u]], dtype=np.float32)
    assert K.replay_sequential(col)[0] == np.float32(1.0) == K.replay_reduce(col, 4)[0]
    assert K.replay_pairwise(col)[0] == np.float32(1.0 + 2.0 ** -23)
    # 8 rows over 4 groups: (r0 + r4) + (r1 + r5) + ... differs from the sequential order
    col8 = np.array([[1.0], [u], [u], [u], [u], [u], [u], [u]], dtype=np.float32)
    assert K.replay_sequential(col8)[0] == np.float32(1.0)
    assert K.replay_reduce(col8, 4)[0] != np.float32(1.0)
