"""seg_sqnorm_kernel and lars_kernel at the layouts a whole model reaches (tests/lars_cases.py;
tests/test_lars_scale_cpu.py shows that the cases reach these loops and that a kernel wrong in
one of them misses the checks below).  Bounds and replay are those of tests/test_lars_gpu.py.

* seg_sqnorm on "wide": the item grid-stride loop with a second item in 626 blocks of the
  2048-block grid (a short item after a full one in blocks 0 .. 112), the last-arrival ticket at
  that grid, the per-tensor finish loop with up to nine trips per lane; every item partial, every
  sum and every trust column bit for bit against the replay.
* seg_sqnorm on "max_segs": the finish's wave loop over 4095 tensors, 2047 blocks with two items.
* lars_kernel on "wide": the LDS table fill over 1905 entries (eight trips), flat_stream at its
  grid cap with a second pass whose quads lie in another tensor than their first-pass aliases;
  "nesterov" runs on the buffer of n % 4 = 3 (the scalar tail through the null segment).
* lars_kernel on "max_segs": the 32 KiB table, entry 4095 the null segment.
* FusedLARS over ResNet-18's parameters (2770 items; 576 of them, nine trips per lane, in the
  largest tensor): two steps on synthetic gradients, every tensor's norms and ratio against the
  replay of the pre-step state, every element against lars_reference's bounds.
"""
import numpy as np
import pytest
import torch

from ddp_amd.ops import FusedLARS
from ddp_amd.ops import kernel_bounds as kb
from lars_cases import COEF, EPS, LAYOUTS, LR, MOM, TC, WD, Layout, too_many_tables, wide_tail
from test_lars_cpu import check_bounds
from test_lars_gpu import G, ISENT, SENT, bits, guarded, guards_intact

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
NULL_ROW = [1.0, 0.0, 0.0, 0.0]


def test_constants_match_the_replay(C):
    assert (C.LARS_ITEM, C.LARS_CHUNK) == (kb.LARS_ITEM, kb.LARS_CHUNK)
    assert (C.LARS_MAX_BLOCKS, C.LARS_MAX_SEGS) == (kb.LARS_MAX_BLOCKS, kb.LARS_MAX_SEGS)


def with_nan_padding(L, x):
    """x on the device with NaN in every padding element between and after the tensors."""
    out = x.clone()
    out[:L.N][torch.from_numpy(~L.inside[:L.N])] = float("nan")
    return out.to(dev)


class Workspace:
    """The plan and seg_sqnorm's outputs, each inside sentinel words (and filled with them)."""

    def __init__(self, C, L, like):
        self.L = L
        self.plan = C.lars_plan(*L.tables(), L.n, like)
        self.pbuf, self.partials = guarded(2 * L.n_items, torch.float32)
        self.tkbuf, self.ticket = guarded(4, torch.int32, ISENT)
        self.ticket[:1] = 0
        self.sbuf, sums = guarded(2 * L.n_seg, torch.float32)
        self.sums = sums.view(L.n_seg, 2)
        self.trbuf, trust = guarded(4 * (L.n_seg + 1), torch.float32)
        self.trust = trust.view(L.n_seg + 1, 4)
        self.trust[L.n_seg] = torch.tensor(NULL_ROW)

    def norms(self, C, w, g, gscale=None):
        C.seg_sqnorm(w, g, self.plan, self.partials, self.ticket, self.sums, self.trust, TC, EPS, gscale)
        torch.cuda.synchronize()

    def check_untouched(self):
        L = self.L
        assert guards_intact(self.pbuf, 2 * L.n_items) and guards_intact(self.sbuf, 2 * L.n_seg)
        assert guards_intact(self.trbuf, 4 * (L.n_seg + 1)), "words around the trust table were written"
        assert self.trust[L.n_seg].tolist() == NULL_ROW, "the null segment was written"
        t = self.tkbuf.cpu()
        assert int(t[G]) == 0, "the ticket is re-armed"
        assert bool((t[:G] == ISENT).all()) and bool((t[G + 1:] == ISENT).all())


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got, dtype=np.float32).view(np.int32),
                          np.ascontiguousarray(want, dtype=np.float32).view(np.int32))


# ------------------------------------------------------------------------------ seg_sqnorm
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", ["wide", "max_segs"])
def test_seg_sqnorm_is_the_replayed_order_bit_for_bit(C, name, clip):
    """Two consecutive launches (the second on another gradient: the ticket re-arms); NaN in every
    padding element; the outputs start as sentinel words, so an item or a tensor that is never
    written shows."""
    L = LAYOUTS[name]
    ws = None
    for launch, seed in enumerate((1, 2)):
        w, g = with_nan_padding(L, L.inputs(1)[0]), with_nan_padding(L, L.inputs(seed)[1])
        wb, gb = bits(w), bits(g)
        ws = ws or Workspace(C, L, w)
        gsb, gs = guarded(4, torch.float32)
        gs.fill_(COEF)
        ws.norms(C, w, g, gs[:1] if clip else None)
        (pw, sw), (pg, sg) = L.replayed(0, 1), L.replayed(1, seed)
        trust = L.trust(sw, sg, COEF if clip else None)
        part = ws.partials.view(L.n_items, 2).cpu().numpy()
        for col, want in enumerate((pw, pg)):
            bad = np.flatnonzero(part[:, col].view(np.int32) != want.view(np.int32))
            assert bad.size == 0, f"launch {launch}: {bad.size} item partials of {'wg'[col]} differ, first item {bad[0]}"
        sums = ws.sums.cpu().numpy()
        assert same_bits(sums[:, 0], sw) and same_bits(sums[:, 1], sg), f"launch {launch}: sums of squares"
        got = ws.trust[:L.n_seg].cpu().numpy()
        for col, what in enumerate(("ratio", "wd", "wn", "gn")):
            bad = np.flatnonzero(got[:, col].view(np.int32) != trust[:, col].view(np.int32))
            assert bad.size == 0, f"launch {launch}: {what} of {bad.size} tensors differs, first tensor {bad[0]}"
        assert got[L.zero_w, 2] == 0.0 and got[L.zero_w, 0] == 1.0 and got[L.zero_g, 3] == 0.0 and got[L.zero_g, 0] == 1.0
        assert (got[np.array(L.excluded), 0] == 1.0).all()
        assert int((got[:, 0] != 1.0).sum()) == sum(L.adapts) - 2
        ws.check_untouched()
        assert torch.equal(bits(w), wb) and torch.equal(bits(g), gb), "w and g are read-only"
        assert guards_intact(gsb, 4) and bool((gs == COEF).all())


# ------------------------------------------------------------------------------ lars_kernel
CASES = {  # layout, nesterov, first, clip, dlr
    "first": ("wide", False, True, False, False), "clip_dlr": ("wide", False, False, True, True),
    "nesterov": ("wide_tail", True, False, False, False), "max_segs": ("max_segs", False, False, True, False),
}
RATES = [0.05, 0.02, 0.08]


@pytest.mark.parametrize("case", list(CASES))
def test_lars_kernel_per_element(C, case):
    """Momentum 0.9.  Every element of p and m within the derived bounds of the float64 rule; a
    bf16 shadow over the whole buffer equals bf16(p) bit for bit; the gradient and the trust table
    are read-only; the padding between the tensors stays zero; with DLR the schedule state
    advanced exactly once."""
    name, nesterov, first, clip, dlr = CASES[case]
    L = wide_tail() if name == "wide_tail" else LAYOUTS[name]
    n = L.n
    w0, g0, m0 = L.inputs(1)
    bufs = [guarded(n + (-n) % 4, torch.float32) for _ in range(3)]
    (pb, p), (gb, g), (mb, m) = [(b, v[:n]) for b, v in bufs]
    for v, h in ((p, w0), (g, g0), (m, torch.zeros(n) if first else m0)):
        v.copy_(h)
    ws = Workspace(C, L, p)
    gsb, gs = guarded(4, torch.float32)
    gs.fill_(COEF)
    ws.norms(C, p, g, gs[:1] if clip else None)
    trust_before = ws.trust.clone()
    shb, sh = guarded(n + (-n) % 4, torch.bfloat16)
    sched = None
    if dlr:
        tbuf, table = guarded(4, torch.float32)
        table[:3] = torch.tensor(RATES)
        sbuf = torch.full((12,), ISENT, dtype=torch.int32, device=dev)
        sbuf[4:8] = torch.tensor([1, 0, 0, 0], dtype=torch.int32)
        sched = (table[:3], sbuf[4:8])
    C.lars(p, g, m, LR, MOM, 0.0, nesterov, False, first, True, [(0, n, sh[:n], 1, 0, 0, 0)], ws.plan, ws.trust,
           gs[:1] if clip else None, sched)
    torch.cuda.synchronize()
    lr = float(np.float32(RATES[1])) if dlr else LR
    segs, wds, adapts = L.segs_ref()
    ref = kb.lars_reference(w0.numpy(), g0.numpy(), None if first else m0.numpy(), segs, wds, adapts, lr, MOM, 0.0,
                            nesterov, False, first, TC, EPS, COEF if clip else None)
    assert ref[0].shape == (n,), "every element is compared"
    check_bounds(p.cpu(), m.cpu(), ref, f"scale kernel {case}")
    for b, _ in bufs:
        assert bool((b[:G] == SENT).all()) and bool((b[G + n:] == SENT).all()), "guard band written"
    assert torch.equal(g.cpu(), g0), "the gradient is read-only"
    assert torch.equal(bits(ws.trust), bits(trust_before)), "the trust table is read-only"
    ws.check_untouched()
    pad = torch.from_numpy(~L.inside[:L.N]).to(dev)
    assert bool((p[:L.N][pad] == 0).all()) and bool((sh[:L.N][pad] == 0).all()), "the padding between tensors stays zero"
    assert bool((m[:L.N][pad] == 0).all())
    assert torch.equal(sh[:n].view(torch.int16), p.to(torch.bfloat16).view(torch.int16)), "shadow != bf16(p)"
    assert guards_intact(shb, n)
    assert guards_intact(gsb, 4) and bool((gs == COEF).all())
    if dlr:  # the counter advanced exactly once, the ticket is re-armed, lr_used is the rate of step 1
        s = sbuf.cpu()
        assert bool((s[:4] == ISENT).all()) and bool((s[8:] == ISENT).all())
        assert (int(s[4]), int(s[5]), int(s[7])) == (2, 0, 0)
        assert s[6:7].view(torch.float32)[0].item() == float(np.float32(RATES[1]))
        assert guards_intact(tbuf, 4) and table[:3].tolist() == [float(np.float32(r)) for r in RATES]


def test_plan_refuses_4096_tensors(C):
    """lars_plan refuses LARS_MAX_SEGS + 1 tensors, and so do the two launchers when handed such
    tables as a plan: nothing is launched."""
    segs, items, cmap, n = too_many_tables()
    w0 = torch.randn(n, generator=torch.Generator().manual_seed(5))
    p, g, m = w0.to(dev), w0.to(dev), w0.to(dev)
    with pytest.raises(RuntimeError, match="4095 tensors, got 4096"):
        C.lars_plan(segs, items, cmap, n, p)
    tkb, ticket = guarded(4, torch.int32, ISENT)
    k = segs.shape[0]
    plan = (segs.to(dev), items.to(dev), cmap.to(dev), n)
    _, partials = guarded(2 * k, torch.float32)
    trust = torch.full((k + 1, 4), SENT, device=dev)
    sums = torch.full((k, 2), SENT, device=dev)
    with pytest.raises(RuntimeError, match="plan table sizes"):
        C.seg_sqnorm(p, g, plan, partials, ticket, sums, trust, TC, EPS, None)
    with pytest.raises(RuntimeError, match="plan table sizes"):
        C.lars(p, g, m, LR, MOM, 0.0, False, False, False, True, [], plan, trust, None, None)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), w0) and torch.equal(m.cpu(), w0), "a refused call launched nothing"
    assert bool((partials == SENT).all()) and bool((trust == SENT).all()) and bool((sums == SENT).all())
    assert bool((tkb == ISENT).all())


# ------------------------------------------------------------------------------ FusedLARS
def test_fused_lars_at_resnet18s_layout():
    """resnet18(num_classes=10)'s parameters, no forward or backward: synthetic gradients (scales
    1 .. 1e-3 by tensor) in the flat gradient buffer, momentum 0.9, weight decay, clipping (which
    engages) and the default exclusion of 1-D tensors; the momentum-initialising step and a
    regular one, each against the pre-step fp32 state."""
    from ddp_amd.models import resnet18

    torch.manual_seed(0)
    model = resnet18(num_classes=10).to(dev)
    opt = FusedLARS(model, lr=LR, momentum=MOM, weight_decay=WD, trust_coef=TC, eps=EPS, max_grad_norm=5.0)
    fs = opt.flat
    L = Layout("resnet18", [fs.numels[n] for n in fs.names], excluded=[len(fs.shapes[n]) <= 1 for n in fs.names])
    assert L.begins == [fs.offsets[n] for n in fs.names] and L.n == fs.numel
    assert L.n_items > kb.LARS_MAX_BLOCKS + 32 and L.seg_items.max() == 576 and sum(L.excluded) > 30
    assert [opt.excluded(n) for n in fs.names] == L.excluded
    fs.bf16_params()
    m = None
    for step in range(2):
        grad = L.make_inputs(10 + step)[1]
        fs.reattach_grads()
        fs.grads.copy_(grad)
        w = fs.params.cpu()
        opt.step()
        torch.cuda.synchronize()
        what = f"FusedLARS resnet18 step {step}"
        assert torch.equal(fs.grads.cpu(), grad), "the gradient is read-only"
        clip = opt.grad_clip_stats()  # read back from the device
        coef = clip["coef"]
        assert 0 < coef < 1 and clip["steps"] == step + 1 == clip["clipped"]
        (_, sw), (_, sg) = L.replay(w.numpy()), L.replay(grad.numpy())
        want = L.trust(sw, sg, coef)
        got = opt._ws[4].cpu().numpy()
        assert got[L.n_seg].tolist() == NULL_ROW, "the null segment was written"
        assert same_bits(opt._ws[3].cpu().numpy(), np.stack([sw, sg], axis=1)), f"{what}: sums of squares"
        for col, name in enumerate(("ratio", "wd", "wn", "gn")):
            bad = np.flatnonzero(got[:L.n_seg, col].view(np.int32) != want[:, col].view(np.int32))
            assert bad.size == 0, f"{what}: {name} of {bad.size} tensors differs, first {fs.names[bad[0]]}"
        stats = opt.trust_stats()
        for i, n in enumerate(fs.names):
            s = stats[n]
            assert (s["ratio"], s["w_norm"], s["g_norm"]) == (float(want[i, 0]), float(want[i, 2]), float(want[i, 3])), n
            if L.excluded[i]:
                assert s["ratio"] == 1.0 and not s["adapted"] and got[i, 1] == 0.0, f"{n}: 1-D, so no ratio and no decay"
        adapted = [i for i in range(L.n_seg) if not L.excluded[i]]
        assert all(want[i, 0] != 1.0 and got[i, 1] == np.float32(WD) for i in adapted)
        ref = kb.lars_reference(w.numpy(), grad.numpy(), None if m is None else m.numpy(), L.segs, L.wds, L.adapts, LR,
                                MOM, 0.0, False, False, step == 0, TC, EPS, coef)
        assert ref[0].shape == (fs.numel,), "every element is compared"
        m = opt.momentum_buffer.cpu()
        check_bounds(fs.params.cpu(), m, ref, what)
        assert torch.equal(fs._bf16.view(torch.int16), fs.params.to(torch.bfloat16).view(torch.int16)), "shadow != bf16(p)"
