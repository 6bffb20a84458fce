"""The float64 references of the non-convolution ResNet kernels (ddp_amd/ops/reference.py)
against torch's own double-precision operators, on the CPU: BatchNorm2d in train mode through
autograd, max_pool2d(return_indices=True), adaptive_avg_pool2d, cross_entropy and ``@``, at two
odd shapes each.  tests/test_resnet_ops_elementwise_gpu.py leans on these references."""
import pytest
import torch
import torch.nn.functional as F

from ddp_amd.ops import reference as R

D = torch.float64
TOL = 1e-12


def randn64(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D)


def close(a, b, tol=TOL):
    assert a.shape == b.shape
    assert ((a - b).abs() <= tol * (1.0 + b.abs())).all(), (a - b).abs().max().item()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("N,H,W,C", [(3, 5, 7, 16), (2, 9, 3, 24)])
@pytest.mark.parametrize("res,relu", [(False, False), (True, False), (False, True), (True, True)])
def test_batchnorm_matches_torch_double(N, H, W, C, res, relu):
    x = randn64(N, H, W, C, seed=1) * 1.5 + 0.3
    r = randn64(N, H, W, C, seed=2) if res else None
    gamma, beta = randn64(C, seed=3).abs() + 0.5, randn64(C, seed=4) * 0.3
    dout = randn64(N, H, W, C, seed=5)
    bn = torch.nn.BatchNorm2d(C, dtype=D).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xr = nchw(x).requires_grad_(True)
    rr = nchw(r).requires_grad_(True) if res else None
    out = bn(xr) + rr if res else bn(xr)
    out = torch.relu(out) if relu else out
    out.backward(nchw(dout))
    # the statistics the kernels are handed (biased variance, eps inside the root)
    x2 = x.reshape(-1, C)
    mean = x2.mean(0)
    invstd = 1.0 / torch.sqrt(((x2 - mean) ** 2).mean(0) + bn.eps)
    y = R.bn_apply64(x, mean, invstd, gamma, beta, r, relu)
    close(y, nhwc(out.detach()))
    d = torch.where(y > 0, dout, torch.zeros_like(dout)) if relu else dout
    b = R.bn_bwd64(d, x, mean, invstd, gamma, float(N * H * W))
    close(b["dx"], nhwc(xr.grad))
    close(b["sum_d"], bn.bias.grad)
    close(b["sum_dxh"], bn.weight.grad)
    if res:
        close(d, nhwc(rr.grad))  # the residual branch receives the masked gradient itself
    xh = (x - mean) * invstd
    close(b["abs_d"], d.abs().reshape(-1, C).sum(0))
    close(b["abs_dxh"], (d * xh).abs().reshape(-1, C).sum(0))
    assert (b["abs_d"] >= b["sum_d"].abs()).all() and (b["abs_dxh"] >= b["sum_dxh"].abs() - 1e-12).all()


def torch_pool(x):
    """torch's max pool on NCHW double: y, window index of its argmax, and autograd's dx."""
    N, H, W, C = x.shape
    xr = nchw(x).requires_grad_(True)
    y, flat = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    OH, OW = y.shape[2], y.shape[3]
    ih, iw = flat // W, flat % W
    oh = torch.arange(OH).view(1, 1, OH, 1)
    ow = torch.arange(OW).view(1, 1, 1, OW)
    k = (ih - (2 * oh - 1)) * 3 + (iw - (2 * ow - 1))
    return xr, y, nhwc(k)


@pytest.mark.parametrize("N,H,W,C", [(2, 7, 5, 8), (1, 9, 9, 16), (2, 1, 1, 8), (2, 2, 4, 8)])
@pytest.mark.parametrize("kind", ["randn", "relu", "quantised"])
def test_maxpool_matches_torch_double(N, H, W, C, kind):
    x = randn64(N, H, W, C, seed=7)
    if kind == "relu":
        x = torch.relu(x)  # zeros: ties everywhere
    elif kind == "quantised":
        x = (x * 2).round().clamp(-2, 2) / 2  # five values: ties among positives
    y, idx, bwd = R.maxpool64(x)
    xr, ty, tk = torch_pool(x)
    assert torch.equal(y, nhwc(ty.detach()))
    assert idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) <= 8
    assert torch.equal(idx, tk)  # first maximum in row-major window order
    if kind != "randn" and H * W > 1:
        # the tie rule decided something: an earlier tap holds the same value as a later one
        win = F.unfold(F.pad(nchw(x), (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(N, C, 9, -1)
        assert ((win == win.max(2, keepdim=True).values).sum(2) > 1).any()
    dy = randn64(*y.shape, seed=8)
    ty.backward(nchw(dy))
    close(bwd(dy), nhwc(xr.grad))
    # float32 routing: at most 4 terms per input pixel, the same values up to fp32 rounding
    d32 = bwd(dy.float(), torch.float32)
    assert d32.dtype == torch.float32
    close(d32.double(), nhwc(xr.grad), 1e-6)


def test_maxpool_tie_rule_on_constant_input():
    """All-equal input: every window's first in-bounds tap wins (4 at the top-left corner,
    3 on the left column, 1 on the top row, 0 inside)."""
    y, idx, bwd = R.maxpool64(torch.ones(1, 5, 5, 8, dtype=D))
    want = torch.tensor([[4, 3, 3], [1, 0, 0], [1, 0, 0]])
    assert torch.equal(idx[0, :, :, 0], want) and bool((y == 1).all())
    dx = bwd(torch.ones(1, 3, 3, 8, dtype=D))
    assert dx.sum().item() == 9 * 8 and dx[0, 0, 0, 0].item() == 1 and dx[0, 4, 4, 0].item() == 0


@pytest.mark.parametrize("N,H,W,C", [(3, 3, 3, 64), (2, 7, 5, 24)])
def test_avgpool_matches_torch_double(N, H, W, C):
    x = randn64(N, H, W, C, seed=9)
    xr = nchw(x).requires_grad_(True)
    ref = F.adaptive_avg_pool2d(xr, 1).flatten(1)
    close(R.avgpool64(x), ref.detach())
    dy = randn64(N, C, seed=10)
    ref.backward(dy)
    close(R.avgpool_bwd64(dy, H, W), nhwc(xr.grad))


@pytest.mark.parametrize("B,C", [(5, 65), (7, 127)])
def test_xent_matches_torch_double(B, C):
    x = randn64(B, C, seed=11) * 3
    x[1] = 2.5          # all logits equal
    x[2] += 1e4         # large offset
    x[3] *= 6           # wide spread
    lab = torch.tensor([0, 63, 64, C - 1, 7, 1, 2][:B])
    xr = x.clone().requires_grad_(True)
    ref = F.cross_entropy(xr, lab)
    ref.backward()
    loss, dl = R.xent64(x, lab)
    close(loss, ref.detach())
    close(dl, xr.grad)
    rows, p = R.xent_rows64(x, lab)
    close(rows, F.cross_entropy(x, lab, reduction="none"))
    close(p, torch.softmax(x, 1))
    close(rows[1], torch.log(torch.tensor(float(C), dtype=D)))
    _, dl3 = R.xent64(x, lab, gscale=0.25)
    close(dl3, xr.grad * B * 0.25)


@pytest.mark.parametrize("M,N,K", [(5, 33, 65), (17, 10, 7)])
def test_gemm_matches_torch_double(M, N, K):
    A, Bm, bias, prior = randn64(M, K, seed=12), randn64(K, N, seed=13), randn64(N, seed=14), randn64(M, N, seed=15)
    close(R.gemm64(A, Bm), A @ Bm)
    close(R.gemm64(A, Bm, bias, 0.37, prior), 0.37 * (A @ Bm) + bias + prior)
    # low-precision operands are widened, never rounded
    Ab = A.to(torch.bfloat16)
    close(R.gemm64(Ab, Bm.float()), Ab.double() @ Bm.float().double())
