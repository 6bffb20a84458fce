"""Global-norm gradient clipping on the GPU: grad_sqnorm_kernel (csrc/kernels/grad_norm.hip)
bit for bit against the float32 replay of its documented order and within the a-priori bound
of float64, torch's coefficient rule, the CLIP build of sgd_kernel against scale-then-SGD, the
whole models, and hipGraph replay with a device-resident coefficient."""
import numpy as np
import pytest
import torch

from ddp_amd.ops import kernel_bounds as kb

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
U = kb.U
SENT = 1234.5  # guard-band fill


@pytest.fixture(scope="module", autouse=True)
def _return_cached_blocks():
    """These tests fill tens of MB with NaN, sentinels and 1e2-magnitude values.  Hand the
    freed blocks back to the driver afterwards, so later tests' torch.empty() buffers do not
    start from this module's bit patterns."""
    yield
    import gc

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def mixed(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.where(rng.random(n) < 0.01, 100.0, 0.01)).astype(np.float32)


class Workspace:
    """partials / ticket / stats inside sentinel guard bands; stats' floats pre-filled with NaN."""

    def __init__(self, C):
        self.nb = C.GRAD_NORM_MAX_BLOCKS
        self.pbuf = torch.full((self.nb + 128,), SENT, device=dev)
        self.sbuf = torch.full((12,), SENT, device=dev)
        self.partials, self.stats = self.pbuf[64:64 + self.nb], self.sbuf[4:8]
        self.stats[:2] = float("nan")
        self.stats[2:] = 0.0  # the int32 counters
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)

    def read(self):
        s = self.stats.cpu()
        i = s.view(torch.int32)
        return s[0].numpy().copy(), s[1].numpy().copy(), int(i[2]), int(i[3])

    def check_guards(self, used):
        assert bool((self.pbuf[:64] == SENT).all()) and bool((self.pbuf[64 + used:] == SENT).all())
        assert bool((self.sbuf[:4] == SENT).all()) and bool((self.sbuf[8:] == SENT).all())
        assert int(self.ticket.item()) == 0, "the last block must re-arm the ticket"


def sizes(C):
    per = C.GRAD_NORM_MAX_BLOCKS * C.GRAD_NORM_THREADS * C.GRAD_NORM_QUADS  # quads per full-grid pass
    return [1, 3, 4, 5, 255, 1027, 4 * (per + 1) + 1, 4 * (2 * per + 1) + 3]


def test_constants_match_the_replay(C):
    assert (C.GRAD_NORM_THREADS, C.GRAD_NORM_QUADS, C.GRAD_NORM_MAX_BLOCKS) == \
        (kb.GN_THREADS, kb.GN_QUADS, kb.GN_MAX_BLOCKS)
    for n in sizes(C) + [0, 4096, 4100, 1 << 33]:
        assert C.grad_norm_blocks(n) == kb.grad_norm_blocks(n), n
    assert [kb.sqnorm_passes(n) for n in sizes(C)[-2:]] == [2, 3]


@pytest.mark.parametrize("idx", range(8))
def test_grad_sqnorm_equals_the_replay_bitwise_and_float64_within_bound(C, idx):
    n = sizes(C)[idx]
    g = mixed(n, 100 + idx)
    ref = float((g.astype(np.float64) ** 2).sum())
    b_sum, b_norm, e_coef = kb.sqnorm_bound(n, ref)
    S = kb.replay_sqnorm(g)
    want_norm = np.sqrt(S)  # numpy's float32 sqrt is correctly rounded
    c = 0.5 * float(want_norm)
    gd = torch.from_numpy(g).to(dev)
    ws = Workspace(C)
    seen = []
    for rep in range(2):  # twice: the ticket is re-armed and the bits repeat
        C.grad_sqnorm(gd, c, ws.partials, ws.ticket, ws.stats)
        torch.cuda.synchronize()
        norm, coef, steps, clipped = ws.read()
        ws.check_guards(C.grad_norm_blocks(n))
        assert norm.tobytes() == np.float32(want_norm).tobytes(), (n, float(norm), float(want_norm))
        assert coef.tobytes() == np.float32(kb.clip_coef32(want_norm, c)).tobytes()
        assert abs(float(norm) - np.sqrt(ref)) <= b_norm, (float(norm), np.sqrt(ref), b_norm)
        assert abs(float(norm) ** 2 - ref) <= b_sum + 3 * U * ref  # (squaring the rounded root: 3 u)
        ref_coef = float(np.float32(c)) / (np.sqrt(ref) + 1e-6)
        assert abs(float(coef) - ref_coef) <= e_coef * ref_coef
        assert (steps, clipped) == (rep + 1, rep + 1)
        seen.append((norm.tobytes(), coef.tobytes()))
    assert seen[0] == seen[1]
    assert torch.equal(gd.cpu(), torch.from_numpy(g)), "the kernel only reads the gradient"


def test_coefficient_rule_and_counters(C):
    n = 1027
    g = mixed(n, 7)
    gd = torch.from_numpy(g).to(dev)
    ws = Workspace(C)
    norm32 = np.sqrt(kb.replay_sqnorm(g))
    expect_clipped = 0
    for k, c in enumerate([0.25 * float(norm32), 4.0 * float(norm32), float(norm32), 1e-3, 1e30]):
        C.grad_sqnorm(gd, c, ws.partials, ws.ticket, ws.stats)
        norm, coef, steps, clipped = ws.read()
        t = (torch.tensor(c, dtype=torch.float32) / (torch.tensor(float(norm)) + 1e-6)).clamp(max=1.0)
        assert norm.tobytes() == np.float32(norm32).tobytes()
        assert coef.tobytes() == t.numpy().tobytes(), (c, float(coef), t.item())
        expect_clipped += int(t.item() < 1.0)
        assert (steps, clipped) == (k + 1, expect_clipped)
    assert 2 <= expect_clipped <= 3  # (c == norm clips only where norm + 1e-6f > norm in fp32)
    z = torch.zeros(5000, device=dev)
    C.grad_sqnorm(z, 1.0, ws.partials, ws.ticket, ws.stats)
    norm, coef, steps, clipped = ws.read()
    assert float(norm) == 0.0 and float(coef) == 1.0 and (steps, clipped) == (6, expect_clipped)
    ws.check_guards(C.grad_norm_blocks(5000))


@pytest.mark.parametrize("momentum,nesterov,wd", [(0.0, False, 0.0), (0.9, False, 0.0), (0.9, True, 0.0),
                                                  (0.9, False, 1e-2), (0.0, False, 1e-2)])
@pytest.mark.parametrize("first", [True, False])
def test_clip_pass_equals_scale_then_sgd_bitwise(C, momentum, nesterov, wd, first):
    n = 256 * 4 * 3 + 7  # several blocks, and an n % 4 tail
    gen = torch.Generator().manual_seed(int(momentum * 10) + 2 * nesterov + 4 * first + (8 if wd else 0))
    p0 = torch.randn(n, generator=gen).to(dev)
    g = (torch.randn(n, generator=gen) * 3).to(dev)
    m0 = torch.randn(n, generator=gen).to(dev)
    gscale = torch.tensor([np.float32(0.337), SENT], device=dev)

    def run(clip):
        p, m = p0.clone(), (m0.clone() if momentum else None)
        sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        grads = g if clip else g * gscale[0]  # torch's fp32 product: one rounding per element
        C.sgd(p, grads, m, 0.05, momentum, 0.0, wd, nesterov, False, first, True, [(0, n, sh, 1, 0, 0, 0)],
              gscale[0:1] if clip else None)
        return p, m, sh

    g_before = g.clone()
    (pa, ma, sa), (pb, mb, sb) = run(True), run(False)
    torch.cuda.synchronize()
    assert torch.equal(g, g_before), "the CLIP pass must not rewrite the gradient"
    assert not torch.equal(pa, p0) and torch.equal(pa, pb) and torch.equal(sa, sb)
    assert torch.equal(sa, pa.to(torch.bfloat16))
    if momentum:
        assert torch.equal(ma, mb)
    # (and the unscaled step differs: the scale is applied)
    pc = p0.clone()
    C.sgd(pc, g, m0.clone() if momentum else None, 0.05, momentum, 0.0, wd, nesterov, False, first, True, [])
    assert not torch.equal(pc, pa)


def _model(kind):
    from ddp_amd.models import SimpleCNN, resnet18

    torch.manual_seed(0)
    if kind == "resnet18":
        m = resnet18(num_classes=10).to(dev)
        x, y = torch.randn(4, 3, 64, 64, device=dev), torch.randint(0, 10, (4,), device=dev)
    else:
        m = SimpleCNN().to(dev)
        x, y = torch.rand(8, 1, 28, 28, device=dev), torch.randint(0, 10, (8,), device=dev)
    return m, x, y


@pytest.mark.parametrize("kind", ["resnet18", "simplecnn"])
def test_whole_model_norm_and_huge_max_norm_is_the_unclipped_step(kind):
    """After backward the device norm is within bound of the float64 norm taken parameter by
    parameter (so the alignment padding of the flat buffer contributes nothing), and a
    max_grad_norm that never clips leaves every parameter bitwise equal to an unclipped run."""
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    a, x, y = _model(kind)
    b, _, _ = _model(kind)
    b.load_state_dict(a.state_dict())
    oa = FusedSGD(a, lr=0.05, momentum=0.9, max_grad_norm=1e30)
    ob = FusedSGD(b, lr=0.05, momentum=0.9)
    assert any(v % 64 for v in oa.flat.numels.values()), "needs parameter sizes that are no multiple of 64"
    for _ in range(2):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            CrossEntropyLoss()(m(x), y).backward()
        sumsq = sum(float((p.grad.double() ** 2).sum()) for p in a.parameters())
        oa.step()
        ob.step()
        st = oa.grad_clip_stats()
        _, b_norm, _ = kb.sqnorm_bound(oa.flat.numel, sumsq)
        assert abs(st["total_norm"] - np.sqrt(sumsq)) <= b_norm, (st, np.sqrt(sumsq), b_norm)
        assert st["coef"] == 1.0 and st["clipped"] == 0
    assert oa.grad_clip_stats()["steps"] == 2
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n
    assert torch.equal(oa.momentum_buffer, ob.momentum_buffer)
    assert (oa.flat._bf16 is None) == (ob.flat._bf16 is None)
    if oa.flat._bf16 is not None:  # (ResNet: the flat bf16 weight copy, rewritten by the same pass)
        assert torch.equal(oa.flat._bf16, ob.flat._bf16)


def test_clipped_step_equals_scaled_gradient_step_on_the_model():
    """A max_grad_norm that clips: parameters equal an unclipped FusedSGD fed grads * coef."""
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    a, x, y = _model("simplecnn")
    b, _, _ = _model("simplecnn")
    b.load_state_dict(a.state_dict())
    oa = FusedSGD(a, lr=0.05, momentum=0.9, max_grad_norm=0.01)
    ob = FusedSGD(b, lr=0.05, momentum=0.9)
    for _ in range(2):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            CrossEntropyLoss()(m(x), y).backward()
        oa.step()
        coef = oa.grad_clip_stats()["coef"]
        assert coef < 1
        ob.flat.reattach_grads()
        from ddp_amd.ops import direct_grad

        direct_grad.flush_fresh(p for p, _ in ob.flat._pairs)
        ob.flat.grads.mul_(torch.tensor(coef, dtype=torch.float32, device=dev))
        ob.step()
    assert torch.equal(oa.flat.params, ob.flat.params)
    assert oa.grad_clip_stats()["clipped"] == 2


def test_graph_replay_reads_the_coefficient_on_the_device():
    """GraphedStep with a small max_grad_norm, 4 replays on different batches, against the same
    steps run eagerly: bitwise-equal parameters and per-step norms, and the norms differ from
    step to step - the coefficient is read from device memory, not baked into the graph."""
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    torch.manual_seed(1)
    xs = [torch.randn(4, 3, 64, 64, device=dev) * (1 + i) for i in range(3)]
    ys = [torch.randint(0, 10, (4,), device=dev) for _ in range(3)]

    def make_step(model):
        opt = FusedSGD(model, lr=0.05, momentum=0.9, max_grad_norm=0.05)
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return step, opt

    torch.manual_seed(0)
    e = resnet18(num_classes=10).to(dev)
    f = resnet18(num_classes=10).to(dev)
    f.load_state_dict(e.state_dict())
    (se, oe), (sf, of) = make_step(e), make_step(f)
    order = [0, 0, 1, 2, 0, 1]  # graphed: 2 warm-up steps on xs[0], then 4 replays
    ne = []
    for i in order:
        le = se(xs[i], ys[i])
        ne.append(oe.grad_clip_stats())
    gf = GraphedStep(sf, (xs[0], ys[0]), warmup=2)
    nf = [None, of.grad_clip_stats()]
    for i in order[2:]:
        lf = gf(xs[i], ys[i])
        nf.append(of.grad_clip_stats())
    torch.cuda.synchronize()
    assert torch.equal(le, lf)
    for k in range(1, len(order)):
        assert nf[k] == ne[k], (k, nf[k], ne[k])  # total_norm, coef, steps, clipped
    replayed = [s["total_norm"] for s in nf[2:]]
    assert len(set(replayed)) == 4 and len({s["coef"] for s in nf[2:]}) == 4, replayed
    assert all(s["coef"] < 1 for s in nf[2:]) and nf[-1]["steps"] == len(order) == nf[-1]["clipped"]
    for (n, pe), (_, pf) in zip(e.named_parameters(), f.named_parameters()):
        assert torch.equal(pe, pf), n
