"""Plain-PyTorch fp32 reference implementations of every fused HIP op, in the
kernels' native layouts (NHWC activations, OHWI conv weights, [out][HW][C] fc
weight).  Used (a) as the numerics oracle of the GPU tests and (b) by nothing
on the GPU path - the HIP kernels are mandatory there (see ``ddp_amd.native``).
The float64 references of the non-convolution ResNet kernels are at the end.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def bf16r(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 and back (what a bf16 activation store does)."""
    return t.to(torch.bfloat16).float()


def _f(t: torch.Tensor) -> torch.Tensor:
    """fp32 view of ``t`` - float64 stays float64 (the exact-fp32 path's oracle)."""
    return t if t.dtype == torch.float64 else t.float()


def nhwc_to_nchw(x):
    return x.permute(0, 3, 1, 2)


def nchw_to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def conv1_relu(x: torch.Tensor, w_ohwi: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """x [B,H,W] fp32 -> NHWC fp32 relu(conv3x3(x)+b); w_ohwi [Cout,3,3,1]."""
    y = F.conv2d(x.unsqueeze(1), w_ohwi.permute(0, 3, 1, 2), b, padding=1)
    return nchw_to_nhwc(torch.relu(y))


def conv3x3(x_nhwc, w_ohwi, b, relu=True):
    y = F.conv2d(nhwc_to_nchw(x_nhwc), w_ohwi.permute(0, 3, 1, 2), b, padding=1)
    if relu:
        y = torch.relu(y)
    return nchw_to_nhwc(y)


def conv3x3_dgrad(dy_nhwc, w_ohwi):
    """dX of a 3x3/s1/p1 conv (NHWC in/out)."""
    dx = F.conv_transpose2d(nhwc_to_nchw(dy_nhwc), w_ohwi.permute(0, 3, 1, 2), padding=1)
    return nchw_to_nhwc(dx)


def conv3x3_wgrad(dy_nhwc, x_nhwc):
    """(dW OHWI, db) of a 3x3/s1/p1 conv."""
    x = _f(nhwc_to_nchw(x_nhwc))
    dy = _f(nhwc_to_nchw(dy_nhwc))
    cin, cout = x.shape[1], dy.shape[1]
    dw = torch.nn.grad.conv2d_weight(x, (cout, cin, 3, 3), dy, padding=1)
    return dw.permute(0, 2, 3, 1).contiguous(), dy.sum(dim=(0, 2, 3))


def conv1_wgrad(dz_nhwc, x):
    """(dW [Cout,3,3,1], db) of conv1 given its pre-activation gradient dZ (NHWC)."""
    dy = _f(nhwc_to_nchw(dz_nhwc))
    dw = torch.nn.grad.conv2d_weight(_f(x.unsqueeze(1)), (dy.shape[1], 1, 3, 3), dy, padding=1)
    return dw.permute(0, 2, 3, 1).contiguous(), dy.sum(dim=(0, 2, 3))


def fc_nhwc(x_nhwc, w_native, b):
    """logits = flatten_nhwc(x) @ w_native.reshape(out,-1).T + b."""
    B = x_nhwc.shape[0]
    return _f(x_nhwc.reshape(B, -1)) @ _f(w_native.reshape(w_native.shape[0], -1)).t() + b


def fc_bwd(dl, x_nhwc, w_native, mask=True):
    """(dX NHWC [masked by X>0], dW native) of fc_nhwc."""
    B = x_nhwc.shape[0]
    xf = _f(x_nhwc.reshape(B, -1))
    wf = _f(w_native.reshape(w_native.shape[0], -1))
    dx = dl @ wf
    if mask:
        dx = dx * (xf > 0)
    dw = dl.t() @ xf
    return dx.view_as(x_nhwc), dw.view_as(w_native)


def cross_entropy(logits, labels, label_smoothing=0.0):
    """(mean loss, dlogits = (softmax - onehot)/B); with ``label_smoothing`` = eps the target is
    (1 - eps) onehot + eps / C over all C classes (torch's)."""
    lp = torch.log_softmax(_f(logits), dim=1)
    loss = F.nll_loss(lp, labels)
    d = lp.exp()
    if label_smoothing:
        eps, C = float(label_smoothing), logits.shape[1]
        loss = (1.0 - eps) * loss + (eps / C) * (-lp.sum(1)).mean()
        d[torch.arange(logits.shape[0]), labels] -= 1.0 - eps
        d -= eps / C
    else:
        d[torch.arange(logits.shape[0]), labels] -= 1.0
    return loss, d / logits.shape[0]


def simple_cnn_step_bf16(params: dict, x: torch.Tensor, labels: torch.Tensor, ws: int = 1,
                         label_smoothing: float = 0.0):
    """fp32 PyTorch model of ONE SimpleCNN training step that rounds to bf16 at exactly
    the points the HIP pipeline stores bf16 (activations, MFMA operands, dZ tensors).

    ``params``: native layouts ``w1 [32,3,3,1]``, ``b1``, ``w2 [64,3,3,32]`` (OHWI),
    ``b2``, ``wfc [10,784,64]``, ``bfc``; ``x`` float [B,28,28] in [0,1].
    Returns (loss, grads dict in native layouts, prescaled by 1/ws).
    """
    B = x.shape[0]
    w1, b1, w2, b2 = params["w1"].float(), params["b1"].float(), params["w2"].float(), params["b2"].float()
    wfc, bfc = params["wfc"].float(), params["bfc"].float()
    w2b, wfcb = bf16r(w2), bf16r(wfc)
    a1 = bf16r(conv1_relu(x.float(), w1, b1))                      # [B,28,28,32]
    a2 = bf16r(conv3x3(a1, w2b, b2, relu=True))                     # [B,28,28,64]
    logits = fc_nhwc(a2, wfcb, bfc)
    loss, dl = cross_entropy(logits, labels, label_smoothing)
    dz2 = bf16r((dl @ wfcb.reshape(wfcb.shape[0], -1)).view_as(a2) * (a2 > 0))
    dwfc = (dl.t() @ a2.reshape(B, -1)).view_as(wfc)
    dw2, db2 = conv3x3_wgrad(dz2, a1)
    dz1 = bf16r(conv3x3_dgrad(dz2, w2b)) * (a1 > 0)
    dw1, db1 = conv1_wgrad(dz1, x.float())
    s = 1.0 / ws
    return loss, {"w1": dw1 * s, "b1": db1 * s, "w2": dw2 * s, "b2": db2 * s,
                  "wfc": dwfc * s, "bfc": dl.sum(0) * s}


def simple_cnn_step_exact(params: dict, x: torch.Tensor, labels: torch.Tensor, ws: int = 1,
                          dtype: torch.dtype = torch.float64, label_smoothing: float = 0.0):
    """The same step without any bf16 rounding, evaluated in ``dtype`` (float64 by
    default): the oracle of the exact-fp32 path (``--dtype fp32``), whose MFMA results
    are plain fp32 fma chains.  Same arguments / returns as :func:`simple_cnn_step_bf16`."""
    B = x.shape[0]
    p = {k: v.to(dtype) for k, v in params.items()}
    w1, b1, w2, b2, wfc, bfc = p["w1"], p["b1"], p["w2"], p["b2"], p["wfc"], p["bfc"]
    x = x.to(dtype)
    a1 = conv1_relu(x, w1, b1)
    a2 = conv3x3(a1, w2, b2, relu=True)
    logits = fc_nhwc(a2, wfc, bfc)
    loss, dl = cross_entropy(logits, labels, label_smoothing)
    dz2 = (dl @ wfc.reshape(wfc.shape[0], -1)).view_as(a2) * (a2 > 0)
    dwfc = (dl.t() @ a2.reshape(B, -1)).view_as(wfc)
    dw2, db2 = conv3x3_wgrad(dz2, a1)
    dz1 = conv3x3_dgrad(dz2, w2) * (a1 > 0)
    dw1, db1 = conv1_wgrad(dz1, x)
    s = 1.0 / ws
    return loss, {"w1": dw1 * s, "b1": db1 * s, "w2": dw2 * s, "b2": db2 * s,
                  "wfc": dwfc * s, "bfc": dl.sum(0) * s}


# ---------------------------------------------------------------------------------------
# float64 CPU references of the non-convolution ResNet kernels (csrc/kernels/resnet_ops.hip,
# xent.hip).  NHWC tensors, the kernels' own inputs (BatchNorm takes mean / invstd / gamma /
# beta as given - nothing is recomputed); every result is unrounded float64.
# tests/test_resnet_ops_reference_cpu.py holds them against torch's own double-precision
# operators, tests/test_resnet_ops_elementwise_gpu.py holds the kernels against them.
def _d(t):
    return None if t is None else t.detach().cpu().double()


def bn_apply64(x, mean, invstd, gamma, beta, res=None, relu=False):
    """y = act(x * sc + (beta - mean * sc) [+ res]) with sc = invstd * gamma; x NHWC."""
    x, mean, invstd, gamma, beta, res = map(_d, (x, mean, invstd, gamma, beta, res))
    sc = invstd * gamma
    y = x * sc + (beta - mean * sc)
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def bn_bwd64(d, x, mean, invstd, gamma, count):
    """BatchNorm backward from the (already masked and summed) upstream gradient ``d``.

    Returns a dict: ``sum_d`` = sum d, ``sum_dxh`` = sum d * xhat per channel, their
    absolute-value companions ``abs_d`` = sum |d| and ``abs_dxh`` = sum |d * xhat| (the
    rounding bounds of the sums), ``xh`` and
    ``dx`` = gamma * invstd / count * (count * d - sum_d - xhat * sum_dxh)."""
    d, x, mean, invstd, gamma = map(_d, (d, x, mean, invstd, gamma))
    C = x.shape[-1]
    xh = (x - mean) * invstd
    d2, q2 = d.reshape(-1, C), (d * xh).reshape(-1, C)
    sd, sq = d2.sum(0), q2.sum(0)
    dx = gamma * invstd / count * (count * d - sd - xh * sq)
    return {"sum_d": sd, "sum_dxh": sq, "abs_d": d2.abs().sum(0), "abs_dxh": q2.abs().sum(0), "xh": xh,
            "dx": dx}


def _pool_taps(H, W):
    """3x3 / s2 / p1 window taps: (k, output rows, output cols, input rows, input cols)."""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for k in range(9):
        kh, kw = divmod(k, 3)
        oh = [o for o in range(OH) if 0 <= 2 * o - 1 + kh < H]
        ow = [o for o in range(OW) if 0 <= 2 * o - 1 + kw < W]
        if oh and ow:
            yield (k, torch.tensor(oh), torch.tensor(ow), torch.tensor([2 * o - 1 + kh for o in oh]),
                   torch.tensor([2 * o - 1 + kw for o in ow]))


def maxpool64(x):
    """3x3 / stride 2 / pad 1 max pool of an NHWC tensor.

    Returns ``(y, idx, bwd)``: the float64 maxima, the window index 0..8 (kh * 3 + kw) of
    the FIRST maximum in row-major window order (torch's tie rule) as int64, and
    ``bwd(d, dtype=torch.float64)`` which routes an upstream gradient [N,OH,OW,C] to the
    input by those indices, summing an input pixel's (at most 4) matches in ascending
    window order kh, kw in ``dtype``."""
    x = _d(x)
    N, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    win = torch.full((9, N, OH, OW, C), float("-inf"), dtype=torch.float64)
    for k, oh, ow, ih, iw in _pool_taps(H, W):
        win[k][:, oh[:, None], ow[None, :]] = x[:, ih[:, None], iw[None, :]]
    y = win.max(0).values
    idx = ((win == y).cumsum(0) == 0).sum(0)  # taps before the first maximum

    def bwd(d, dtype=torch.float64):
        d = d.detach().cpu().to(dtype)
        dx = torch.zeros(N, H, W, C, dtype=dtype)
        zero = torch.zeros((), dtype=dtype)
        for k, oh, ow, ih, iw in _pool_taps(H, W):  # ascending k: kh, then kw
            sel = torch.where(idx[:, oh[:, None], ow[None, :]] == k, d[:, oh[:, None], ow[None, :]], zero)
            dx[:, ih[:, None], iw[None, :]] += sel
        return dx

    return y, idx, bwd


def avgpool64(x):
    """Global average pool [N,H,W,C] -> [N,C]."""
    x = _d(x)
    return x.reshape(x.shape[0], -1, x.shape[-1]).sum(1) / (x.shape[1] * x.shape[2])


def avgpool_bwd64(dy, H, W):
    """[N,C] -> [N,H,W,C]: every pixel receives dy / (H * W)."""
    dy = _d(dy)
    return (dy / (H * W))[:, None, None, :].expand(dy.shape[0], H, W, dy.shape[1]).contiguous()


def xent_rows64(logits, labels, label_smoothing=0.0):
    """Per-row softmax cross-entropy: (loss [B], softmax p [B,C]).  ``label_smoothing`` = eps:
    the target is (1 - eps) onehot + eps / C over all C classes (torch's), so the row loss is
    logsumexp(x) - (1 - eps) x_y - (eps / C) sum_c x_c, written here from that definition."""
    x = _d(logits)
    lab = labels.detach().cpu().long()
    z = x - x.max(1, keepdim=True).values
    lse = z.exp().sum(1).log()
    zl = z[torch.arange(x.shape[0]), lab]
    if not label_smoothing:
        return lse - zl, (z - lse[:, None]).exp()
    eps = float(label_smoothing)
    return lse - ((1.0 - eps) * zl + (eps / x.shape[1]) * z.sum(1)), (z - lse[:, None]).exp()


def xent64(logits, labels, gscale=None, label_smoothing=0.0):
    """(mean loss, dlogits = (softmax - (1 - eps) onehot - eps / C) * gscale); gscale defaults
    to 1 / B, eps = ``label_smoothing`` to 0."""
    loss, p = xent_rows64(logits, labels, label_smoothing)
    B, C = p.shape
    d = p.clone()
    if label_smoothing:
        eps = float(label_smoothing)
        d[torch.arange(B), labels.detach().cpu().long()] -= 1.0 - eps
        d -= eps / C
    else:
        d[torch.arange(B), labels.detach().cpu().long()] -= 1.0
    return loss.mean(), d * (1.0 / B if gscale is None else gscale)


def gemm64(A, B, bias=None, alpha=1.0, prior=None):
    """alpha * A @ B [+ bias over columns] [+ prior]; A [M,K], B [K,N]."""
    out = alpha * (_d(A) @ _d(B))
    if bias is not None:
        out = out + _d(bias)
    if prior is not None:
        out = out + _d(prior)
    return out


# ---------------------------------------------------------------------------------------
# float64 CPU references of the SimpleCNN step kernels (conv3x3.hip, conv1.hip, linear.hip,
# optim.hip), written tap by tap from the definition - independent of torch's convolution
# operators, against which tests/test_simplecnn_kernel_bounds_cpu.py holds them.  NHWC
# activations, OHWI weights.
def _shift(x, dh, dw):
    """x [B,H,W,C] -> x at pixel (h + dh, w + dw), zero outside the image."""
    B, H, W, C = x.shape
    out = torch.zeros_like(x)
    h0, h1, w0, w1 = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
    if h0 < h1 and w0 < w1:
        out[:, h0:h1, w0:w1] = x[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
    return out


def conv3x3_64(x, w_ohwi, bias=None, relu=False):
    """y[n,h,w,co] = sum_{kh,kw,ci} x[n,h+kh-1,w+kw-1,ci] w[co,kh,kw,ci] (+ bias), float64."""
    x, w, bias = _d(x), _d(w_ohwi), _d(bias)
    y = torch.zeros(*x.shape[:3], w.shape[0], dtype=torch.float64)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        y += torch.einsum("nhwi,oi->nhwo", _shift(x, kh - 1, kw - 1), w[:, kh, kw, :])
    if bias is not None:
        y = y + bias
    return torch.relu(y) if relu else y


def conv3x3_dgrad64(dy, w_ohwi):
    """dx[n,h,w,ci] = sum_{kh,kw,co} dy[n,h+1-kh,w+1-kw,co] w[co,kh,kw,ci], float64."""
    dy, w = _d(dy), _d(w_ohwi)
    dx = torch.zeros(*dy.shape[:3], w.shape[3], dtype=torch.float64)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        dx += torch.einsum("nhwo,oi->nhwi", _shift(dy, 1 - kh, 1 - kw), w[:, kh, kw, :])
    return dx


def conv3x3_wgrad64(dy, x, rows=None, image=None):
    """(dW OHWI [Co,3,3,Ci], db [Co]) in float64, of output rows [rows[0], rows[1]) of one
    image only when given (one split-K slab row of conv3x3_wgrad)."""
    dy, x = _d(dy), _d(x)
    if image is not None:
        dy, x = dy[image:image + 1], x[image:image + 1]
    if rows is not None:
        keep = torch.zeros_like(dy)
        keep[:, rows[0]:rows[1]] = 1.0
        dy = dy * keep
    dw = torch.zeros(dy.shape[3], 3, 3, x.shape[3], dtype=torch.float64)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        dw[:, kh, kw, :] = torch.einsum("nhwo,nhwi->oi", dy, _shift(x, kh - 1, kw - 1))
    return dw, dy.sum(dim=(0, 1, 2))


def conv1_64(x, w_o9, bias, relu=True):
    """conv1: x [B,H,W] (float, or uint8 read as x / 255) -> relu(conv3x3 + bias) [B,H,W,Co]."""
    xd = _d(x) / 255.0 if x.dtype == torch.uint8 else _d(x)
    return conv3x3_64(xd.unsqueeze(-1), _d(w_o9).reshape(-1, 3, 3, 1), bias, relu)


def conv1_wgrad64(dz, x, pixels=None):
    """(dW [Co,9], db [Co]) of conv1 from dZ [B,H,W,Co]; `pixels` = (p0, p1) restricts the sum
    to the flattened pixels [p0, p1) (one slab row of conv1_wgrad / of the fused dgrad)."""
    dz = _d(dz)
    xd = _d(x) / 255.0 if x.dtype == torch.uint8 else _d(x)
    if pixels is not None:
        keep = torch.zeros(dz.shape[0] * dz.shape[1] * dz.shape[2], dtype=torch.float64)
        keep[pixels[0]:pixels[1]] = 1.0
        dz = dz * keep.view(*dz.shape[:3], 1)
    dw, db = conv3x3_wgrad64(dz, xd.unsqueeze(-1))
    return dw.reshape(dw.shape[0], 9), db


def fc64(x_nhwc, w_native, bias=None):
    """logits [B,NO] = flatten_nhwc(x) . w [NO,HW,C] (+ bias), float64."""
    x, w = _d(x_nhwc), _d(w_native)
    out = x.reshape(x.shape[0], -1) @ w.reshape(w.shape[0], -1).t()
    return out if bias is None else out + _d(bias)


def fc_block_partials64(y_nhwc, w_native, CH):
    """The fused conv2 + fc epilogue's partial logits [blocks][2][NO] in float64: block k
    covers the flattened pixels [k CH, (k + 1) CH); slot 0 is the image of its first pixel,
    slot 1 the next image; a slot whose image the block does not touch is 0."""
    y, w = _d(y_nhwc), _d(w_native)
    B, H, W, C = y.shape
    HW, NO = H * W, w.shape[0]
    yf, wf = y.reshape(B * HW, C), w.reshape(NO, HW, C)
    nblk = -(-B * HW // CH)
    part = torch.zeros(nblk, 2, NO, dtype=torch.float64)
    for k in range(nblk):
        p0, p1 = k * CH, min((k + 1) * CH, B * HW)
        n0 = p0 // HW
        for slot in (0, 1):
            a, b = max(p0, (n0 + slot) * HW), min(p1, (n0 + slot + 1) * HW)
            if a < b:
                part[k, slot] = torch.einsum("pc,opc->o", yf[a:b], wf[:, a - (n0 + slot) * HW:b - (n0 + slot) * HW])
    return part


def fc_bwd64(dl, x_nhwc, w_native, scale=1.0, mask=True):
    """(dX [masked by x > 0], dW * scale, dbias * scale) of fc64, float64."""
    dl, x, w = _d(dl), _d(x_nhwc), _d(w_native)
    B = x.shape[0]
    xf = x.reshape(B, -1)
    dx = dl @ w.reshape(w.shape[0], -1)
    if mask:
        dx = dx * (xf > 0)
    return dx.view_as(x), scale * (dl.t() @ xf).view_as(w), scale * dl.sum(0)


def sgd64(p, g, m, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, maximize=False, first_step=False):
    """One torch.optim.SGD step (torch/optim/sgd.py _single_tensor_sgd) in float64:
    returns (new parameter, new momentum buffer or None)."""
    p, g, m = _d(p), _d(g), _d(m)
    d = -g if maximize else g
    if wd != 0.0:
        d = d + wd * p
    buf = None
    if momentum != 0.0:
        buf = d.clone() if first_step else momentum * m + (1.0 - dampening) * d
        d = d + momentum * buf if nesterov else buf
    return p - lr * d, buf
