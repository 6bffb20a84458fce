"""The SMOOTH builds of the cross-entropy kernels on MI355X (xent_wave_rows_kernel<true>,
xent_kernel<true>, both csrc/kernels/xent.hip; ``C.xent(..., label_smoothing=e)``), per element against the float64
reference within the a-priori bounds that tests/test_label_smoothing_cpu.py derives
(tests/label_smoothing_cases.py computes them), and end to end through
``CrossEntropyLoss(label_smoothing=)``: SimpleCNN's module path against the CPU model, and
ResNet-18's captured step graph against its eager step.  Outputs are NaN-prefilled and
guarded as in tests/test_resnet_ops_elementwise_gpu.py.  Run with -s for the LS_RATIO lines."""
import pytest
import torch

import label_smoothing_cases as LS
from ddp_amd.ops import reference as R
from elementwise import F32, Guarded, bits

pytestmark = pytest.mark.gpu
dev = "cuda"


def held(name, shape, out, ref, bound, what):
    ok, r = LS.within(out, ref, bound)
    print(f"LS_RATIO {name} {shape} {r:.4f}")
    assert ok, f"{what}: {name} error / bound = {r:.3f} (or unwritten / non-finite elements)"


def run(C, lg, lab, eps, what, G=1, part=None, bias=None, want_extras=False, dbias_scale=0.0):
    """One launch through the binding on guarded outputs; returns (dlogits, loss, logits_out, dbias)."""
    B, NC = lg.shape
    g = LS.f32(1.0 / B)
    dl, loss = Guarded((B, NC), F32), Guarded((1,), F32)
    lo = Guarded((B, NC), F32) if want_extras else None
    db = Guarded((NC,), F32) if want_extras else None
    kw = {} if eps is None else {"label_smoothing": eps}
    C.xent(lg if part is None else part, G, bias, lab, lo.t if lo else None, dl.t, loss.t, db.t if db else None, g,
           dbias_scale, **kw)
    torch.cuda.synchronize()
    for o in (dl, loss, lo, db):
        if o is not None:
            o.check(what)
    return dl.t, loss.t, lo.t if lo else None, db.t if db else None


def check_against_reference(lg, lab, eps, dl, loss, name, what):
    B, NC = lg.shape
    e, g = LS.f32(eps), LS.f32(1.0 / B)
    loss_ref, dl_ref, bl, bd = LS.bounds(lg, lab, e, g)
    held(name + "_dlogits", (B, NC, eps), dl, dl_ref, bd, what)
    held(name + "_loss", (B, NC, eps), loss, loss_ref, bl, what)
    rs = dl.detach().cpu().double().sum(1).abs()
    assert bool((rs <= bd.sum(1)).all()), f"{what}: a row of dlogits does not sum to zero within the bound"


# ------------------------------------------------------------------------------ wave kernel
@pytest.mark.parametrize("B,NC", [(1, 65), (4, 1000), (5, 1000), (7, 1024), (9, 127)])
@pytest.mark.parametrize("eps", [0.1, 1.0])
def test_wave_kernel_smooth(C, B, NC, eps):
    """One wave per row: one class past a lane row, a full and a ragged last block of 4 rows,
    every register step used, and a class count that is no multiple of 64."""
    lg, lab = (t.to(dev) for t in LS.xent_inputs(B, NC))
    what = f"xent wave {(B, NC)} eps={eps}"
    dl, loss, _, _ = run(C, lg, lab, eps, what)
    check_against_reference(lg, lab, eps, dl, loss, "wave", what)
    _, loss2, _, _ = run(C, lg, lab, eps, what)
    assert torch.equal(bits(loss), bits(loss2)), f"{what}: the loss is not run-to-run identical"


# ----------------------------------------------------------------------------- block kernel
@pytest.mark.parametrize("eps", [0.1, 1.0])
def test_block_kernel_smooth(C, eps):
    lg, lab = (t.to(dev) for t in LS.xent_inputs(7, 10))
    what = f"xent block (7, 10) eps={eps}"
    dl, loss, _, _ = run(C, lg, lab, eps, what)
    check_against_reference(lg, lab, eps, dl, loss, "block", what)
    dl32, loss32, _, _ = run(C, lg, lab.to(torch.int32), eps, what + " int32 labels")
    assert torch.equal(bits(dl), bits(dl32)) and torch.equal(bits(loss), bits(loss32)), \
        f"{what}: the two label sources disagree"
    _, loss2, _, _ = run(C, lg, lab, eps, what)
    assert torch.equal(bits(loss), bits(loss2)), f"{what}: the loss is not run-to-run identical"


@pytest.mark.parametrize("eps", [0.1, 1.0])
@pytest.mark.parametrize("ldtype", [torch.int64, torch.int32])
def test_block_kernel_smooth_with_partials_bias_logits_and_dbias(C, eps, ldtype):
    """G = 3 partials + bias, logits_out and the fused dbias (B = 5, C = 10; four waves, so wave 0
    owns rows 0 and 4): the logits the kernel stores are the reference's input, they do not
    depend on eps, and dbias is the in-order sum of the stored smoothed dlogits."""
    B, G, NC, scale = 5, 3, 10, 0.25
    gen = torch.Generator().manual_seed(71)
    part = (torch.randn(B, G, NC, generator=gen) * 0.7).to(dev)
    bias = (torch.randn(NC, generator=gen) * 0.2).to(dev)
    lab = torch.tensor([NC - 1, 0, 3, 7, 3], dtype=ldtype, device=dev)
    what = f"xent block G=3 eps={eps} {ldtype}"
    shape = torch.empty(B, NC)  # (run() takes B and the class count from it; the input is `part`)
    dl, loss, lo, db = run(C, shape, lab, eps, what, G=G, part=part, bias=bias, want_extras=True, dbias_scale=scale)
    _, _, lo0, _ = run(C, shape, lab, None, what, G=G, part=part, bias=bias, want_extras=True, dbias_scale=scale)
    assert torch.equal(bits(lo), bits(lo0)), f"{what}: logits_out depends on label_smoothing"
    x = part.cpu()
    lref = ((x[:, 0] + x[:, 1]) + x[:, 2]) + bias.cpu()  # the kernel's order: 0 + partials in turn, then the bias
    assert torch.equal(bits(lo), bits(lref)), f"{what}: logits_out"
    check_against_reference(lo, lab.long(), eps, dl, loss, "block_g3", what)
    d = dl.cpu()
    want = ((((d[0] + d[4]) + d[1]) + d[2]) + d[3]) * torch.tensor(scale, dtype=F32)
    assert torch.equal(bits(db), bits(want)), f"{what}: dbias is not the in-order sum of the stored dlogits"


# ------------------------------------------------------------------------------- eps = 0
@pytest.mark.parametrize("B,NC", [(5, 1000), (9, 127), (7, 10)])
def test_explicit_zero_is_the_call_without_the_keyword(C, B, NC):
    lg, lab = (t.to(dev) for t in LS.xent_inputs(B, NC))
    what = f"xent {(B, NC)} eps=0"
    dl, loss, _, _ = run(C, lg, lab, None, what)
    dl0, loss0, _, _ = run(C, lg, lab, 0.0, what)
    assert torch.equal(bits(dl), bits(dl0)) and torch.equal(bits(loss), bits(loss0))
    dls, _, _, _ = run(C, lg, lab, 0.1, what)
    assert not torch.equal(bits(dl), bits(dls))  # (the keyword is not ignored)


# ----------------------------------------------------------------------------- end to end
def test_simple_cnn_module_path_with_label_smoothing_matches_references():
    """tests/test_kernels_gpu.py::test_simple_cnn_module_path_matches_references with
    label_smoothing = 0.1 on both sides and B = 8: the same comparisons and tolerances."""
    from ddp_amd.models import SimpleCNN
    from ddp_amd.ops import CrossEntropyLoss

    eps, B = 0.1, 8
    torch.manual_seed(0)
    cpu = SimpleCNN()
    gpu = SimpleCNN().to(dev)
    gpu.load_state_dict(cpu.state_dict())
    g0 = torch.Generator().manual_seed(25)
    x = torch.rand(B, 1, 28, 28, generator=g0)
    y = torch.randint(0, 10, (B,), generator=g0)
    loss_c = torch.nn.functional.cross_entropy(cpu(x), y, label_smoothing=eps)
    loss_c.backward()
    loss_g = CrossEntropyLoss(label_smoothing=eps)(gpu(x.to(dev)), y.to(dev))
    loss_g.backward()
    assert abs(loss_g.item() - loss_c.item()) < 2e-2
    plain = torch.nn.functional.cross_entropy(cpu(x), y).item()
    assert abs(loss_c.item() - plain) > 10 * 1e-4  # (the 1e-4 below tells the smoothed loss from the plain one)

    def relclose(a, b, tol):
        a, b = a.float().cpu(), b.float().cpu()
        err = (a - b).norm() / b.norm().clamp_min(1e-12)
        assert err < tol, f"relative error {err:.3e}"

    def native(m):
        return {"w1": m.net[0].weight.detach(), "b1": m.net[0].bias.detach(), "w2": m.net[2].weight.detach(),
                "b2": m.net[2].bias.detach(), "wfc": m.fl.weight.detach(), "bfc": m.fl.bias.detach()}

    pe = {k: v.detach().cpu() for k, v in native(cpu).items()}
    _, g_b = R.simple_cnn_step_bf16(pe, x.view(B, 28, 28), y, label_smoothing=eps)
    _, g_x = R.simple_cnn_step_exact(pe, x.view(B, 28, 28), y, label_smoothing=eps)
    key = {"net.0.weight": "w1", "net.0.bias": "b1", "net.2.weight": "w2", "net.2.bias": "b2",
           "fl.weight": "wfc", "fl.bias": "bfc"}
    for (n, pc), (_, pg) in zip(cpu.named_parameters(), gpu.named_parameters()):
        k = key[n]
        e_k = ((g_b[k].double() - g_x[k]).norm() / g_x[k].norm()).item()
        relclose(pg.grad, pc.grad, 1.25 * e_k + 1e-3)
    p = {k: v.cpu() for k, v in native(gpu).items()}
    loss_e, ge = R.simple_cnn_step_bf16(p, x.view(B, 28, 28), y, label_smoothing=eps)
    assert abs(loss_g.item() - loss_e.item()) < 1e-4
    grads = {"w1": gpu.net[0].weight.grad, "b1": gpu.net[0].bias.grad, "w2": gpu.net[2].weight.grad,
             "b2": gpu.net[2].bias.grad, "wfc": gpu.fl.weight.grad, "bfc": gpu.fl.bias.grad}
    for k in ge:
        relclose(grads[k], ge[k], 1e-2)


def test_resnet18_graphed_step_with_label_smoothing_equals_eager():
    """ResNet-18 at 64 x 64, 16 classes, batch 4: three eager steps against three steps through
    the captured step graph (one warm-up step, two replays) with label_smoothing = 0.1 -
    bitwise-equal losses, parameters and buffers: the value travels by value into the capture."""
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    gen = torch.Generator().manual_seed(5)
    xs = [torch.randn(4, 3, 64, 64, generator=gen).to(dev) for _ in range(3)]
    ys = [torch.randint(0, 16, (4,), generator=gen).to(dev) for _ in range(3)]

    def make_step(model, eps):
        opt = FusedSGD(model, lr=0.05, momentum=0.9, weight_decay=1e-4)
        lossf = CrossEntropyLoss(label_smoothing=eps)

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return step

    torch.manual_seed(0)
    e = resnet18(num_classes=16).to(dev)
    f = resnet18(num_classes=16).to(dev)
    z = resnet18(num_classes=16).to(dev)
    f.load_state_dict(e.state_dict())
    z.load_state_dict(e.state_dict())
    se, sf, sz = make_step(e, 0.1), make_step(f, 0.1), make_step(z, 0.0)
    le = [se(xs[i], ys[i]).clone() for i in range(3)]
    gf = GraphedStep(sf, (xs[0], ys[0]), warmup=1)  # the warm-up step is step 0
    lf = [gf.warmup_out.clone()] + [gf(xs[i], ys[i]).clone() for i in (1, 2)]
    l0 = sz(xs[0], ys[0])
    torch.cuda.synchronize()
    for a, b in zip(le, lf):
        assert torch.equal(a, b), (le, lf)
    assert all(bool(torch.isfinite(v)) for v in le)
    assert not torch.equal(le[0], l0), "label_smoothing = 0.1 left the loss where 0 has it"
    for (n, pe), (_, pf) in zip(e.named_parameters(), f.named_parameters()):
        assert torch.equal(pe, pf), n
    for (n, be), (_, bf) in zip(e.named_buffers(), f.named_buffers()):
        assert torch.equal(be, bf), n
