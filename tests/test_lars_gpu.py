"""LARS on the GPU: seg_sqnorm_kernel bit for bit against the numpy replay of its documented
order, lars_kernel per element against the float64 rule under the derived bounds
(tests/test_lars_cpu.py, whose docstring holds the derivation), the SGD anchor, hipGraph replay,
the bindings' operand checks and the CLI."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ddp_amd.ops import FusedLARS, FusedSGD, LRSchedule
from ddp_amd.ops import kernel_bounds as kb
from ddp_amd.ops.lars import lars_layout
from elementwise import Guarded, bits
from test_lars_cpu import (ADAPTS, BEGINS, COEF, EPS, LENS, LR, MOM, N, SEGS, TC, WDS, ZERO_G, ZERO_W, check_bounds,
                           make_inputs)

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 1234.5   # guard-band fill (exact in bf16 and fp32)
ISENT = 0x5A5A5A5A
G = 64          # guard elements on each side (a multiple of 4: 16-byte alignment kept)
NSEG = len(LENS)
NITEMS = sum(kb.lars_items(m) for m in LENS)


def guarded(n, dtype, fill=SENT):
    g = Guarded(n, dtype, fill, dev, guard=G, sentinel=fill)  # (the view starts as sentinel too)
    return g.buf, g.t


def guards_intact(buf, n, fill=SENT):
    return bool((buf[:G] == fill).all()) and bool((buf[G + n:] == fill).all())


def with_nan_padding(x):
    """x on the device with NaN in every padding element (between and after the tensors)."""
    out = torch.full((N,), float("nan"), device=dev)
    for b, n in SEGS:
        out[b:b + n] = x[b:b + n].to(dev)
    return out


@functools.lru_cache(maxsize=None)
def inputs(seed=1):
    return make_inputs(seed)


class Workspace:
    """The plan and seg_sqnorm's outputs, each inside sentinel words."""

    def __init__(self, C, like, n=N):
        self.plan = C.lars_plan(*lars_layout(BEGINS, LENS, n, WDS, ADAPTS), n, like)
        self.pbuf, self.partials = guarded(2 * NITEMS, torch.float32)
        self.tkbuf, self.ticket = guarded(4, torch.int32, ISENT)
        self.ticket[:1] = 0
        self.sbuf, sums = guarded(2 * NSEG, torch.float32)
        self.sums = sums.view(NSEG, 2)
        self.trbuf, trust = guarded(4 * (NSEG + 1), torch.float32)
        self.trust = trust.view(NSEG + 1, 4)
        self.trust[NSEG] = torch.tensor([1.0, 0.0, 0.0, 0.0])

    def norms(self, C, w, g, gscale=None):
        C.seg_sqnorm(w, g, self.plan, self.partials, self.ticket, self.sums, self.trust, TC, EPS, gscale)
        torch.cuda.synchronize()

    def check_untouched(self):
        assert guards_intact(self.pbuf, 2 * NITEMS) and guards_intact(self.sbuf, 2 * NSEG)
        assert guards_intact(self.trbuf, 4 * (NSEG + 1)), "words around the trust table were written"
        assert self.trust[NSEG].tolist() == [1.0, 0.0, 0.0, 0.0], "the null segment was written"
        t = self.tkbuf.cpu()
        assert int(t[G]) == 0, "the ticket is re-armed"
        assert bool((t[:G] == ISENT).all()) and bool((t[G + 1:] == ISENT).all())


def expected_norms(w, g, coef=None):
    """(sums [NSEG, 2], trust [NSEG, 4]) float32 from the numpy replay and the fp32 formula."""
    sums, trust = np.zeros((NSEG, 2), np.float32), np.zeros((NSEG, 4), np.float32)
    for i, (b, n) in enumerate(SEGS):
        sums[i] = (kb.replay_seg_sqnorm(w[b:b + n].numpy()), kb.replay_seg_sqnorm(g[b:b + n].numpy()))
        wn, gn, ratio = kb.trust_ratio32(sums[i, 0], sums[i, 1], WDS[i], TC, EPS, ADAPTS[i], coef)
        trust[i] = (ratio, WDS[i], wn, gn)
    return sums, trust


# ------------------------------------------------------------------------------ seg_sqnorm
@pytest.mark.parametrize("clip", [False, True])
def test_seg_sqnorm_is_the_replayed_order_bit_for_bit(C, clip):
    """Lengths 1, 3, 4, 5, 63, 64, 65, one item, one item + 1, three items + 7; one all-zero w, one
    all-zero g; NaN in every padding element.  Two consecutive launches (the second on another
    gradient) show that the ticket re-arms."""
    w0, g0, _ = inputs()
    ws = None
    for launch, gh in enumerate((g0, make_inputs(2)[1])):
        w, g = with_nan_padding(w0), with_nan_padding(gh)
        wb, gb = bits(w), bits(g)
        ws = ws or Workspace(C, w)
        gsb, gs = guarded(4, torch.float32)
        gs.fill_(COEF)
        ws.norms(C, w, g, gs[:1] if clip else None)
        sums, trust = expected_norms(w0, gh, COEF if clip else None)
        assert np.array_equal(bits(ws.sums).numpy(), sums.view(np.int32)), f"launch {launch}: sums of squares"
        got = ws.trust[:NSEG].cpu().numpy()
        for col, name in enumerate(("ratio", "wd", "wn", "gn")):
            assert np.array_equal(got[:, col].view(np.int32), trust[:, col].view(np.int32)), f"launch {launch}: {name}"
        assert got[ZERO_W, 2] == 0.0 and got[ZERO_W, 0] == 1.0 and got[ZERO_G, 3] == 0.0 and got[ZERO_G, 0] == 1.0
        assert all(got[i, 0] == 1.0 for i in range(NSEG) if not ADAPTS[i])
        assert sum(got[i, 0] != 1.0 for i in range(NSEG)) == sum(ADAPTS) - 2
        ws.check_untouched()
        assert torch.equal(bits(w), wb) and torch.equal(bits(g), gb), "w and g are read-only"
        assert guards_intact(gsb, 4) and bool((gs == COEF).all())
        # per-item partials: the last tensor's four items sum (in order) to its total
        part = ws.partials.view(NITEMS, 2)[-4:, 0].cpu().numpy()
        lanes = [np.float32(p) for p in part]  # four lanes, one partial each, then the wave tree
        assert np.float32(np.float32(lanes[0] + lanes[1]) + np.float32(lanes[2] + lanes[3])) == sums[-1, 0]


# ------------------------------------------------------------------------------ lars_kernel
CASES = {  # momentum, nesterov, first, maximize, clip, dlr, tail
    "mom0": (0.0, False, False, False, False, False, 0), "mom": (MOM, False, False, False, False, False, 0),
    "first": (MOM, False, True, False, False, False, 0), "nesterov": (MOM, True, False, False, False, False, 0),
    "maximize": (MOM, False, False, True, False, False, 0), "clip": (MOM, False, False, False, True, False, 0),
    "dlr": (MOM, False, False, False, False, True, 0), "clip_dlr": (MOM, True, False, False, True, True, 0),
    "tail": (MOM, False, False, False, False, False, 3),
}
RATES = [0.05, 0.02, 0.08]


@pytest.mark.parametrize("case", list(CASES))
def test_lars_kernel_per_element(C, case):
    """Every element of p and m within the derived bounds of the float64 rule; a plain bf16 shadow
    over the whole buffer and a PAD4 shadow over the 63-element tensor equal bf16(p) bit for bit.
    "tail": a buffer of N + 3 elements, whose last three (padding: the null segment) go through
    the scalar tail as plain SGD."""
    mom, nesterov, first, maximize, clip, dlr, tail = CASES[case]
    w0, g0, m0 = (torch.cat([x, 0.5 * torch.ones(tail)]) for x in inputs())
    n = N + tail
    segs_ref = SEGS + ([(N, tail)] if tail else [])
    bufs = [guarded(n + (-n) % 4, torch.float32) for _ in range(3)]
    (pb, p), (gb, g), (mb, m) = [(b, v[:n]) for b, v in bufs]
    for v, h in ((p, w0), (g, g0), (m, torch.zeros(n) if first else m0)):
        v.copy_(h)
    ws = Workspace(C, p, n)
    gsb, gs = guarded(4, torch.float32)
    gs.fill_(COEF)
    ws.norms(C, p, g, gs[:1] if clip else None)
    trust_before = ws.trust.clone()
    shb, sh = guarded(n + (-n) % 4, torch.bfloat16)
    b4, n4 = SEGS[4]
    padb, pad = guarded(n4 // 3 * 4, torch.bfloat16)
    shadows = [(0, n, sh[:n], 1, 0, 0, 0), (b4, n4, pad, 4, 0, 0, 0)]
    sched = None
    if dlr:
        tbuf, table = guarded(4, torch.float32)
        table[:3] = torch.tensor(RATES)
        sbuf = torch.full((12,), ISENT, dtype=torch.int32, device=dev)
        sbuf[4:8] = torch.tensor([1, 0, 0, 0], dtype=torch.int32)
        sched = (table[:3], sbuf[4:8])
    C.lars(p, g, m if mom else None, LR, mom, 0.0, nesterov, maximize, first, True, shadows, ws.plan, ws.trust,
           gs[:1] if clip else None, sched)
    torch.cuda.synchronize()
    lr = float(np.float32(RATES[1])) if dlr else LR
    ref = kb.lars_reference(w0.numpy(), g0.numpy(), None if (first or not mom) else m0.numpy(), segs_ref,
                            WDS + [0.0] * bool(tail), ADAPTS + [False] * bool(tail), lr, mom, 0.0, nesterov, maximize,
                            first, TC, EPS, COEF if clip else None)
    check_bounds(p.cpu(), m.cpu() if mom else None, ref, f"kernel {case}")
    if not mom:
        assert torch.equal(m.cpu(), m0), "without momentum the buffer is not touched"
    for b, _ in bufs:
        assert bool((b[:G] == SENT).all()) and bool((b[G + n:] == SENT).all()), "guard band written"
    assert torch.equal(g.cpu(), g0), "the gradient is read-only"
    assert torch.equal(bits(ws.trust), bits(trust_before)), "the trust table is read-only"
    ws.check_untouched()
    for i, (b, k) in enumerate(SEGS):  # padding inside the buffer (zero p, zero g: the null segment) stays zero
        end = BEGINS[i + 1] if i + 1 < NSEG else N
        assert bool((p[b + k:end] == 0).all()) and bool((sh[b + k:end] == 0).all())
    assert torch.equal(sh[:n], p.to(torch.bfloat16)), "shadow != bf16(p)"
    assert guards_intact(shb, n)
    assert torch.equal(pad.view(-1, 4)[:, :3], p[b4:b4 + n4].to(torch.bfloat16).view(-1, 3)), "PAD4 shadow"
    assert bool((pad.view(-1, 4)[:, 3] == SENT).all()) and guards_intact(padb, n4 // 3 * 4)
    if dlr:  # the counter advanced exactly once, the ticket is re-armed, lr_used is the rate of step 1
        s = sbuf.cpu()
        assert bool((s[:4] == ISENT).all()) and bool((s[8:] == ISENT).all())
        assert (int(s[4]), int(s[5]), int(s[7])) == (2, 0, 0)
        assert s[6:7].view(torch.float32)[0].item() == float(np.float32(RATES[1]))
        assert guards_intact(tbuf, 4)
        C.lars(p, g, m, LR, mom, 0.0, nesterov, maximize, False, True, [], ws.plan, ws.trust,
               gs[:1] if clip else None, sched)
        torch.cuda.synchronize()
        s = sbuf.cpu()
        assert (int(s[4]), int(s[5])) == (3, 0) and s[6:7].view(torch.float32)[0].item() == float(np.float32(RATES[2]))


def test_update_false_rewrites_shadows_only(C):
    w0, g0, m0 = inputs()
    p, g, m = (x.to(dev) for x in (w0, g0, m0))
    ws = Workspace(C, p)
    ws.norms(C, p, g)
    shb, sh = guarded(N, torch.bfloat16)
    state = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=dev)
    C.lars(p, g, m, LR, MOM, 0.0, False, False, False, False, [(0, N, sh, 1, 0, 0, 0)], ws.plan, ws.trust, None,
           (torch.tensor(RATES, device=dev), state))
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), w0) and torch.equal(m.cpu(), m0)
    assert torch.equal(sh, p.to(torch.bfloat16)) and guards_intact(shb, N)
    assert state.tolist() == [1, 0, 0, 0], "a shadows-only launch is no optimizer step"


# ------------------------------------------------------------------------------ FusedLARS
def _simplecnn():
    from ddp_amd.models import SimpleCNN

    torch.manual_seed(0)
    return SimpleCNN().to(dev)


def _step_fn(model, opt):
    from ddp_amd.ops import CrossEntropyLoss

    lossf = CrossEntropyLoss()

    def step(x, y):
        opt.zero_grad()
        loss = lossf(model(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


def _batches(k):
    g = torch.Generator().manual_seed(11)
    return [(torch.rand(8, 1, 28, 28, generator=g).to(dev), torch.randint(0, 10, (8,), generator=g).to(dev))
            for _ in range(k)]


def test_sgd_anchor_bit_for_bit():
    """Every tensor excluded and the uniform decay forced: FusedLARS steps are FusedSGD steps bit
    for bit in parameters, momentum and the bf16 shadow."""
    wd = 1e-2
    outs = []
    for kind in ("lars", "sgd"):
        model = _simplecnn()
        if kind == "lars":
            opt = FusedLARS(model, lr=LR, momentum=MOM, weight_decay=wd, exclude=lambda name, shape: True,
                            max_grad_norm=0.5)
            opt._excluded_wd = wd
        else:
            opt = FusedSGD(model, lr=LR, momentum=MOM, weight_decay=wd, max_grad_norm=0.5)
        fs = opt.flat
        fs.bf16_params()
        gen = torch.Generator().manual_seed(3)
        for _ in range(2):  # the momentum-initialising step and a regular one
            fs.reattach_grads()
            for n in fs.names:
                fs.view(fs.grads, n).copy_(torch.randn(fs.shapes[n], generator=gen))
            opt.step()
        torch.cuda.synchronize()
        outs.append((fs.params.clone(), opt.momentum_buffer.clone(), fs._bf16.clone()))
        if kind == "lars":
            assert all(v["ratio"] == 1.0 and not v["adapted"] for v in opt.trust_stats().values())
    for a, b, what in zip(*outs, ("parameters", "momentum", "bf16 shadow")):
        raw = torch.int32 if a.dtype == torch.float32 else torch.int16
        assert torch.equal(a.view(raw), b.view(raw)), what


def test_captured_graph_follows_the_ratios():
    """SimpleCNN's module path at batch 8 in a GraphedStep with clipping and a schedule: 1 warm-up
    step + 5 replays are bitwise 6 eager steps, and the ratios read after each replay differ from
    step to step and equal the eager run's - a graph that froze them cannot pass."""
    from ddp_amd.engine import GraphedStep

    rates = [0.4, 0.8, 0.6, 0.3, 0.5, 0.2]
    data = _batches(6)

    def run(graphed):
        model = _simplecnn()
        opt = FusedLARS(model, lr=rates[0], momentum=MOM, weight_decay=1e-3, trust_coef=0.02, max_grad_norm=0.05,
                        lr_schedule=LRSchedule.from_values(rates))
        step = _step_fn(model, opt)
        ratios = []
        if graphed:
            gs = GraphedStep(step, data[0], warmup=1)
            torch.cuda.synchronize()
            ratios.append(opt.trust_stats()["fl.weight"]["ratio"])
            for x, y in data[1:]:
                gs(x, y)
                torch.cuda.synchronize()
                ratios.append(opt.trust_stats()["fl.weight"]["ratio"])
            assert gs.replays == 5
        else:
            for x, y in data:
                step(x, y)
                ratios.append(opt.trust_stats()["fl.weight"]["ratio"])
        torch.cuda.synchronize()
        return opt, opt.flat.params.clone(), opt.momentum_buffer.clone(), ratios

    og, pg, mg, rg = run(True)
    oe, pe, me, re_ = run(False)
    assert torch.equal(pg, pe) and torch.equal(mg, me), "replays did not follow the eager steps"
    assert rg == re_ and len(set(rg[1:])) == 5, rg
    assert og.schedule_step() == 6 == oe.schedule_step()
    assert og.grad_clip_stats() == oe.grad_clip_stats() and og.grad_clip_stats()["steps"] == 6
    assert og.trust_stats() == oe.trust_stats()


def test_bindings_refuse_wrong_operands(C):
    w0, g0, m0 = inputs()
    p, g, m = (x.to(dev) for x in (w0, g0, m0))
    ws = Workspace(C, p)
    seg = lambda **kw: C.seg_sqnorm(kw.get("p", p), kw.get("g", g), kw.get("plan", ws.plan), ws.partials, ws.ticket,
                                    ws.sums, kw.get("trust", ws.trust), TC, EPS, None)
    upd = lambda **kw: C.lars(kw.get("p", p), kw.get("g", g), kw.get("m", m), LR, MOM, 0.0, False, False, False, True,
                              [], kw.get("plan", ws.plan), kw.get("trust", ws.trust), None, kw.get("sched"))
    big_p, big_g = torch.zeros(N + 4, device=dev), torch.zeros(N + 4, device=dev)
    for call in (seg, upd):
        with pytest.raises(RuntimeError, match="dtype"):
            call(g=g.double())
        with pytest.raises(RuntimeError, match="GPU tensor"):
            call(p=w0.clone())
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(p=big_p[1:N + 1], g=big_g[1:N + 1])
        with pytest.raises(RuntimeError, match="trust"):
            call(trust=ws.trust[:NSEG])
        with pytest.raises(RuntimeError, match="built for a flat buffer"):
            call(p=big_p, g=big_g)
        with pytest.raises(RuntimeError):
            call(plan=None)
    with pytest.raises(RuntimeError, match="momentum"):
        upd(m=m[:N - 4])
    with pytest.raises(RuntimeError, match="sched"):
        upd(sched=(torch.tensor(RATES, device=dev), torch.zeros(4, device=dev)))
    segs, items, cmap = lars_layout(BEGINS, LENS, N, WDS, ADAPTS)
    bad_items = items.clone()
    bad_items[-1, 1] = 4096  # the last piece would run past its tensor
    with pytest.raises(RuntimeError, match="work item"):
        C.lars_plan(segs, bad_items, cmap, N, p)
    bad_map = cmap.clone()
    bad_map[3] = NSEG + 1
    with pytest.raises(RuntimeError, match="cmap"):
        C.lars_plan(segs, items, bad_map, N, p)
    with pytest.raises(RuntimeError, match="inside the flat buffer"):
        C.lars_plan(segs, items, cmap[:-1], N - 64, p)
    with pytest.raises(RuntimeError, match="int32"):
        C.lars_plan(segs.long(), items, cmap, N, p)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), w0) and torch.equal(m.cpu(), m0), "a refused call launched nothing"


# ------------------------------------------------------------------------------------ CLI
def _cli(args, cwd, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, "-u", os.path.join(REPO, "train_ddp.py"), "--world_size", "1", "--device", "gpu",
           "--optimizer", "lars", "--log_every", "1", *args]
    p = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return p.stdout


def test_cli_resnet18_graph_module_lars(tmp_path):
    mj = tmp_path / "metrics.jsonl"
    out = _cli(["--model", "resnet18", "--image_size", "64", "--num_classes", "10", "--dataset_size", "64",
                "--batch_size", "16", "--graph_module", "--epochs", "2", "--momentum", "0.9", "--lr", "0.5",
                "--weight_decay", "1e-4", "--trust_coef", "0.02", "--clip_grad_norm", "5", "--lr_schedule", "cosine",
                "--warmup_steps", "2", "--metrics_json", str(mj), "--checkpoint_dir", str(tmp_path / "ck")], tmp_path)
    losses = [float(ln.rsplit("Loss:", 1)[1]) for ln in out.splitlines() if "| Loss:" in ln]
    assert len(losses) >= 2 and bool(torch.isfinite(torch.tensor(losses)).all())
    recs = [json.loads(ln) for ln in mj.read_text().splitlines()]
    assert len(recs) == 2
    for r in recs:
        assert 0 < r["trust_ratio_min"] <= r["trust_ratio_max"] and r["trust_ratio_max"] != 1.0
    osd = torch.load(tmp_path / "ck" / "epoch_1.pt", weights_only=True)["optimizer"]
    from ddp_amd.models import resnet18

    params = [torch.nn.Parameter(torch.zeros_like(s["momentum_buffer"])) for s in osd["state"].values()]
    assert len(params) == len(list(resnet18(num_classes=10).parameters()))
    topt = torch.optim.SGD(params, lr=0.1)
    topt.load_state_dict(osd)
    assert topt.param_groups[0]["momentum"] == 0.9 and osd["param_groups"][0]["trust_coef"] == 0.02
    assert torch.equal(topt.state[params[0]]["momentum_buffer"], osd["state"][0]["momentum_buffer"])
