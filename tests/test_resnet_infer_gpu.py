"""The inference epilogue of every forward convolution path, and the evaluation tail kernel,
per element on MI355X.

conv_gemm_infer computes  out = bf16(relu?(acc * sc[co] + sh[co] (+ res)))  with acc the fp32
accumulator of the convolution (csrc/kernels/conv_infer.h).  Every path a forward result can
leave a kernel by is compared with a float64 CPU reference of relu?(conv(x, w) * sc + sh + res)
on the bf16 operands the kernel sees, element by element, against an a-priori bound (nothing
calibrated on the kernels).  With u = 2**-24, K the accumulated terms of one output element
and A = conv(|x|, |w|):

    |out - ref| <= 2**-8 |ref|                         the one bf16 store
                 + (K + 2) u |sc| A                    the fp32 accumulation (any order, split K
                                                       partials re-summed), scaled by sc
                 + 3 u (|acc sc| + |sh| + |res|)       the epilogue's fma and add

sc / sh differ per channel and carry, inside one lane's group of 4 consecutive channels, a
negative, a zero and a large entry, so a channel mis-indexed within the group cannot pass.
Every output, split-K workspace and residual is carved out of a larger buffer with sentinel
bands on both sides (nothing outside is written) and outputs / workspaces are pre-filled with
NaN (every element is written).  Run with -s for the INFER_RATIO <path> <geometry> <error /
bound> lines; profiles/resnet_eval/README.md records the largest per path.

Tail kernel (resnet_eval_tail): pred / correct / correct5 exactly equal a plain
implementation of the stated rules; the per-row loss is held to the wave-per-row cross-entropy
bound of tests/test_resnet_ops_elementwise_gpu.py: (D + 64) u max(1, |ref|), D = max |x - max|.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from elementwise import BF, Guarded, U, f64, nchw, nhwc, rnd

pytestmark = pytest.mark.gpu
dev = "cuda"


def affine(Cout, seed):
    """Per-channel sc / sh (fp32, what the kernel reads) with the special entries."""
    g = torch.Generator().manual_seed(seed)
    sc = torch.randn(Cout, generator=g) * 0.5 + 1.0
    sh = torch.randn(Cout, generator=g) * 0.3
    sc[1], sc[2], sc[3] = -0.75, 0.0, 40.0          # one lane's 4-channel group: all different
    sc[Cout - 2], sc[Cout - 1] = 17.0, -3.0
    sh[4], sh[5], sh[6] = -2.0, 0.0, 100.0
    sh[Cout - 1] = 9.0
    return sc.to(dev), sh.to(dev)


class Case:
    """Inputs and float64 references of one convolution (computed once per geometry)."""

    def __init__(self, N, H, W, Cin, Cout, K, s, p, seed=0):
        self.geo = (N, H, W, Cin, Cout, K, s, p)
        self.OH, self.OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        self.x = rnd(N, H, W, Cin, relu=True, seed=seed + 1)
        self.w = rnd(Cout, K, K, Cin, scale=0.05, seed=seed + 2)
        if Cin == 4:  # stem operands: the 4th channel is the zero padding
            self.x[..., 3] = 0
            self.w[..., 3] = 0
        self.res = rnd(N, self.OH, self.OW, Cout, scale=1.5, seed=seed + 3)
        self.sc, self.sh = affine(Cout, seed + 4)
        xd, wd = nchw(self.x), nchw(self.w)
        self.acc = nhwc(F.conv2d(xd, wd, stride=s, padding=p))
        self.A = nhwc(F.conv2d(xd.abs(), wd.abs(), stride=s, padding=p))
        self.K = K * K * Cin


_CASES = {}


def case(*geo):
    if geo not in _CASES:
        _CASES[geo] = Case(*geo)
    return _CASES[geo]


def run(C, cv, family, res, relu, bp=0, bc=0, splits=0, halo=-1, want_halo=None, want_split=None):
    N, H, W, Cin, Cout, K, s, p = cv.geo
    y = Guarded((N, cv.OH, cv.OW, Cout), BF)
    pbp, pbc, sp, _, _, hl = C.conv_gemm_plan(cv.x, y.t, K, K, s, p, False, bp, bc, splits, -1, halo)
    if want_halo is not None:
        assert hl == want_halo, (cv.geo, hl)
    if want_split is not None:
        assert (sp > 1) == want_split, (cv.geo, sp)
    part = Guarded((sp * y.t.numel(),), torch.float32) if sp > 1 else None
    rg = Guarded(tuple(cv.res.shape), BF, cv.res) if res else None
    C.conv_gemm_infer(cv.x, cv.w, cv.sc, cv.sh, rg.t if rg else None, y.t, K, K, s, p, relu,
                      part.t if part else None, bp, bc, splits, halo)
    torch.cuda.synchronize()
    what = f"{family} {cv.geo} res={res} relu={relu} plan bp={pbp} bc={pbc} splits={sp} halo={hl}"
    sc, sh = cv.sc.cpu().double(), cv.sh.cpu().double()
    rd = cv.res.cpu().double() if res else torch.zeros_like(cv.acc)
    pre = cv.acc * sc + sh + rd
    ref = torch.relu(pre) if relu else pre
    bound = (2.0 ** -8 * ref.abs() + (cv.K + 2) * U * sc.abs() * cv.A
             + 3 * U * ((cv.acc * sc).abs() + sh.abs() + rd.abs()) + 1e-30)
    o = f64(y.t)
    assert bool(torch.isfinite(o).all()), f"{what}: unwritten / non-finite elements"
    rr = (o - ref).abs() / bound
    r = rr.max().item()
    print(f"INFER_RATIO {family} {cv.geo} res={int(res)} relu={int(relu)} {r:.4f}")
    if r > 1.0:
        i = tuple(int(v) for v in torch.nonzero(rr == rr.max())[0])
        what += f" at {i}: out {o[i].item()!r} ref {ref[i].item()!r}; {int((rr > 1).sum())} elements out of bound"
    assert r <= 1.0, f"{what}: error / bound = {r:.3f}"
    for g_ in (y, part, rg):
        if g_ is not None:
            g_.check(what)
    if part is not None:
        assert bool(torch.isfinite(part.t).all()), f"{what}: unwritten split-K partials"
    if rg is not None:
        assert torch.equal(rg.t, cv.res), f"{what}: the residual was written"
    return r


@pytest.mark.parametrize("res,relu", [(True, True), (False, True), (False, False)])
def test_gathered_3x3_s2(C, res, relu):
    """Gathered 3x3 / s2, 9x9 -> 5x5, 32 -> 64 channels: 50 pixels, a partial 64-pixel tile."""
    run(C, case(2, 9, 9, 32, 64, 3, 2, 1), "gemm_3x3s2", res, relu, want_halo=0, want_split=False)


def test_pointwise_s2_downsample(C):
    """1x1 / s2, 10x6 -> 5x3, 64 -> 128 channels, no ReLU, no residual (the downsample use)."""
    run(C, case(2, 10, 6, 64, 128, 1, 2, 0), "gemm_1x1s2", False, False, want_halo=0, want_split=False)


@pytest.mark.parametrize("H,W", [(5, 13), (14, 14)])
@pytest.mark.parametrize("res", [True, False])
def test_halo_3x3_s1(C, H, W, res):
    """The LDS halo tile, forced: 5 rows x 13 wide (runtime width, partial last row group) and
    14 x 14 (the width-specialised build), 64 -> 64 channels, N = 2."""
    run(C, case(2, H, W, 64, 64, 3, 1, 1), "halo", res, True, splits=1, halo=1, want_halo=1, want_split=False)


def test_split_k_reduce(C):
    """7x7, 512 -> 512 channels: the planner splits K on its own; the affine, the residual and
    the ReLU are applied to the fp32 sum in the split-K reduction."""
    run(C, case(1, 7, 7, 512, 512, 3, 1, 1), "splitk", True, True, want_split=True)


@pytest.mark.parametrize("H,W", [(45, 45), (30, 50)])
def test_gathered_stem(C, H, W):
    run(C, case(1, H, W, 4, 64, 7, 2, 3), "stem_gathered", False, True)


def test_staged_stem_224(C):
    run(C, case(1, 224, 224, 4, 64, 7, 2, 3), "stem_staged", False, True)


def test_bn_fold_is_bn_affine(C):
    """sc = rsqrt(var + eps) * gamma within 3 ulp = 6 u of float64 (the sum and the product round
    to half an ulp each, the device rsqrt to at most 2), sh = fma(-mean, sc, beta) within one
    rounding of the value computed from that sc, and sc exactly 0 / sh exactly beta where gamma is zero."""
    g = torch.Generator().manual_seed(3)
    Cc = 96
    mean, var = torch.randn(Cc, generator=g) * 0.5, torch.rand(Cc, generator=g) * 1.5 + 0.5
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    gamma[7] = 0.0
    sc, sh = Guarded((Cc,), torch.float32), Guarded((Cc,), torch.float32)
    C.bn_fold(mean.to(dev), var.to(dev), gamma.to(dev), beta.to(dev), 1e-5, sc.t, sh.t)
    torch.cuda.synchronize()
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    sc_ref = gamma.double() / torch.sqrt(var.double() + eps)
    assert bool(((sc.t.cpu().double() - sc_ref).abs() <= 6 * U * sc_ref.abs()).all())
    sh_ref = beta.double() - mean.double() * sc.t.cpu().double()
    assert bool(((sh.t.cpu().double() - sh_ref).abs() <= 2 * U * (beta.abs() + (mean * sc.t.cpu()).abs()).double()).all())
    assert sc.t[7].item() == 0.0 and sh.t[7].item() == beta[7].item()
    sc.check("bn_fold sc")
    sh.check("bn_fold sh")


# --------------------------------------------------------------------------- tail kernel
def rules(row, label):
    """pred, correct, correct5 of one row by the stated rules, in plain Python."""
    x = row.tolist()
    if any(math.isnan(v) for v in x):
        pred = 0
    else:
        mx = max(x)
        pred = min(j for j, v in enumerate(x) if v == mx)
    xl = x[label]
    before = sum(1 for j, v in enumerate(x) if v > xl or (v == xl and j < label))
    return pred, int(pred == label), int(before < 5)


def tail_rows(NC, group):
    """B = 3 rows of NC classes and their labels."""
    g = torch.Generator().manual_seed(100 + NC)
    lg = torch.randn(3, NC, generator=g) * 3
    lab = [0, 0, 0]
    last = NC - 1
    if group == "max":
        # an exact tie for the maximum (two classes, the label the higher one: pred != label);
        # the label equal to the (single) maximum; a row whose maximum is NaN
        lg[0, last] = lg[0, 1] = 50.0
        lab[0] = last
        lg[1, min(65, last)] = 60.0
        lab[1] = min(65, last)
        lg[2, min(2, last)] = float("nan")
        lab[2] = 0
    else:
        # the label tied with another class at the 5th / 6th place, on both sides of the index
        # rule: 4 classes above, then the tied pair (with <= 5 classes: tied at the bottom)
        top = [0, 1, 2, 3] if NC > 5 else [0]
        a, b = (last - 1, last) if NC > 5 else (1, 2)
        for r in (0, 1):
            lg[r] = torch.randn(NC, generator=g)
            for k, j in enumerate(top):
                lg[r, j] = 30.0 + k
            lg[r, a] = lg[r, b] = 20.0
        lab[0], lab[1] = a, b          # lower index: 5th (hit); higher index: 6th (miss when NC > 5)
        lab[2] = int(lg[2].argmax())   # a plain row
    return lg.to(dev), torch.tensor(lab, dtype=torch.int64, device=dev)


@pytest.mark.parametrize("NC", [1000, 10, 4])
@pytest.mark.parametrize("group", ["max", "rank"])
def test_eval_tail(C, NC, group):
    lg, lab = tail_rows(NC, group)
    B = lg.shape[0]
    pred, corr, c5 = (Guarded((B,), torch.int32, torch.full((B,), -7, dtype=torch.int32)) for _ in range(3))
    loss = Guarded((B,), torch.float32)
    C.resnet_eval_tail(lg, lab, pred.t, loss.t, corr.t, c5.t)
    torch.cuda.synchronize()
    what = f"tail NC={NC} {group}"
    want = [rules(lg[r].cpu(), int(lab[r])) for r in range(B)]
    assert pred.t.tolist() == [w[0] for w in want], what
    assert corr.t.tolist() == [w[1] for w in want], what
    assert c5.t.tolist() == [w[2] for w in want], what
    if group == "rank":
        assert c5.t.tolist()[:2] == ([1, 0] if NC > 5 else [1, 1])  # (the cases are what they claim)
    else:
        assert want[0][:2] == (1, 0) and want[1][1] == 1 and want[2][0] == 0
    x = lg.cpu().double()
    for r in range(B):
        got = loss.t[r].item()
        if bool(torch.isnan(x[r]).any()):
            assert math.isnan(got), what
            continue
        ref = (torch.logsumexp(x[r], 0) - x[r, int(lab[r])]).item()
        D = (x[r] - x[r].max()).abs().max().item()
        bound = (D + 64) * U * max(1.0, abs(ref))
        print(f"INFER_RATIO tail_loss ({NC}, {group}, row {r}) {abs(got - ref) / bound:.4f}")
        assert abs(got - ref) <= bound, f"{what} row {r}: loss {got!r} ref {ref!r} bound {bound:.3e}"
    for g_ in (pred, corr, c5, loss):
        g_.check(what)


def test_eval_totals_continue_in_index_order(C):
    """Two calls continue one running (top-1, top-5, fp64 loss) total: the sums of the rows."""
    g = torch.Generator().manual_seed(9)
    n = 1500  # more than one 1024-row chunk
    c1 = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).to(dev)
    c5 = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).to(dev)
    ls = torch.rand(n, generator=g).to(dev)
    tot = torch.zeros(2, dtype=torch.int64, device=dev)
    tl = torch.zeros(1, dtype=torch.float64, device=dev)
    C.resnet_eval_totals(c1, c5, ls, 1100, tot, tl)
    C.resnet_eval_totals(c1[1100:], c5[1100:], ls[1100:], n - 1100, tot, tl)
    torch.cuda.synchronize()
    assert tot.tolist() == [int(c1.sum()), int(c5.sum())]
    assert tl.item() == float(ls.cpu().double().cumsum(0)[-1])
