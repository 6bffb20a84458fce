"""Learning-rate schedules on the GPU: the DLR build of sgd_kernel (csrc/kernels/optim.hip) bit
for bit against the by-value kernel, its in-launch step counter, FusedSGD(lr_schedule=) eagerly
and under hipGraph replay, and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ddp_amd.ops.lr_schedule import LRSchedule

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 1234.5   # guard-band fill (exact in bf16 and fp32)
ISENT = 0x5A5A5A5A
G = 64          # guard elements on each side (a multiple of 4: 16-byte alignment kept)
RATES = [0.05, 0.0125, 0.2]  # a, b, c


def guarded(n, dtype):
    buf = torch.full((n + 2 * G,), SENT, dtype=dtype, device=dev)
    return buf, buf[G:G + n]


def guards_intact(buf, n):
    return bool((buf[:G] == SENT).all()) and bool((buf[G + n:] == SENT).all())


class Sched:
    """(table, state) for C.sgd's ``sched``, each inside sentinel words of its own allocation."""

    def __init__(self, rates):
        self.n = len(rates)
        self.tbuf, self.table = guarded(self.n + (-self.n) % 4, torch.float32)
        self.table = self.table[:self.n]
        self.table.copy_(torch.tensor(rates, dtype=torch.float32))
        self.sbuf = torch.full((12,), ISENT, dtype=torch.int32, device=dev)
        self.state = self.sbuf[4:8]
        self.state.zero_()

    def arg(self):
        return (self.table, self.state)

    def read(self):
        s = self.sbuf.cpu()
        assert bool((s[:4] == ISENT).all()) and bool((s[8:] == ISENT).all()), "words around the state were written"
        assert int(s[7]) == 0, "SchedState is three words"
        t = self.tbuf.cpu()
        assert bool((t[:G] == SENT).all()) and bool((t[G + self.n:] == SENT).all()), "the table is read-only"
        return int(s[4]), int(s[5]), s[6:7].view(torch.float32)[0].item()


BIG = 4 * 256 * 2048 + 4 * 256 + 3  # the 2048-block grid cap and a second grid-stride pass, n % 4 = 3
OPTIONS = [  # momentum, weight decay, nesterov, bf16 shadow
    (0.0, 0.0, False, False), (0.9, 0.0, False, False), (0.0, 1e-2, False, False),
    (0.9, 1e-2, False, False), (0.9, 0.0, True, False), (0.9, 1e-2, False, True),
]


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n", [3, 4, 7, 1029, BIG])
def test_dlr_kernel_equals_the_by_value_kernel_bitwise(C, n, clip):
    """5 consecutive launches over a 3-entry table [a, b, c]: after every launch the parameters,
    the momentum buffer and the shadow are bitwise those of C.sgd(lr = a | b | c | c | c) on the
    same inputs; then t == 5, the ticket is re-armed, lr_used == c, and nothing outside the
    buffers was written.  ``clip``: the same with a device-resident gradient scale (<true, true>)."""
    table32 = torch.tensor(RATES, dtype=torch.float32)
    for oi, (mom, wd, nesterov, shadow) in enumerate(OPTIONS):
        gen = torch.Generator().manual_seed(1000 * oi + n % 997)
        p0 = torch.randn(n, generator=gen)
        m0 = torch.randn(n, generator=gen)
        grads = [(torch.randn(n, generator=gen) * (1 + k)).to(dev) for k in range(5)]
        gscale = torch.tensor([np.float32(0.337), SENT], device=dev)
        bufs = {}
        for side in ("dlr", "ref"):
            pb, p = guarded(n, torch.float32)
            mb, m = guarded(n, torch.float32)
            sb, sh = guarded(n, torch.bfloat16)
            p.copy_(p0)
            m.copy_(m0)
            bufs[side] = (pb, p, mb, m, sb, sh)
        sc = Sched(RATES)
        for k in range(5):
            for side in ("dlr", "ref"):
                _, p, _, m, _, sh = bufs[side]
                lr = 999.0 if side == "dlr" else table32[min(k, 2)].item()  # (by value: ignored by the DLR build)
                C.sgd(p, grads[k], m if mom else None, lr, mom, 0.0, wd, nesterov, False, k == 0, True,
                      [(0, n, sh, 1, 0, 0, 0)] if shadow else [], gscale[0:1] if clip else None,
                      sc.arg() if side == "dlr" else None)
            torch.cuda.synchronize()
            (_, pa, _, ma, _, sa), (_, pr, _, mr, _, sr) = bufs["dlr"], bufs["ref"]
            what = (n, clip, OPTIONS[oi], k)
            assert torch.equal(pa, pr), what
            assert torch.equal(ma, mr), what
            assert torch.equal(sa, sr), what
            if shadow:
                assert torch.equal(sa, pa.to(torch.bfloat16)), what
        assert not torch.equal(bufs["dlr"][1].cpu(), p0)
        t, ticket, lr_used = sc.read()
        assert (t, ticket) == (5, 0), what
        assert lr_used == table32[2].item(), what
        for side in ("dlr", "ref"):
            pb, _, mb, m, sb, _ = bufs[side]
            assert guards_intact(pb, n) and guards_intact(mb, n) and guards_intact(sb, n), (what, side)
            if not mom:
                assert torch.equal(m.cpu(), m0), "no momentum: the buffer is not touched"
        assert torch.equal(gscale.cpu(), torch.tensor([np.float32(0.337), SENT]))


@pytest.mark.parametrize("n", [7, 1029 * 4 + 1])
def test_counter_is_exact_over_300_launches(C, n):
    """One block and several: every launch advances t by exactly one and re-arms the ticket."""
    assert (n == 7) == (((n >> 2) + 255) // 256 <= 1)
    p = torch.zeros(n, device=dev)
    g = torch.ones(n, device=dev)
    rates = [2.0 ** -(k % 5) for k in range(300)]  # exact in fp32, as are the sums below
    sc = Sched(rates)
    for _ in range(300):
        C.sgd(p, g, None, 0.0, 0.0, 0.0, 0.0, False, False, False, True, [], None, sc.arg())
    torch.cuda.synchronize()
    t, ticket, lr_used = sc.read()
    assert (t, ticket) == (300, 0)
    assert lr_used == rates[-1]
    assert torch.equal(p.cpu(), torch.full((n,), -sum(rates)))  # each launch used its own entry, once


@pytest.mark.parametrize("n", [1027, 1031])
def test_shadows_only_launch_still_advances_the_sgd_schedule(C, n):
    """sgd_kernel<.., true> with update = False (the binding allows it; FusedSGD never issues it):
    parameters and momentum untouched, the shadow written, and - unlike adamw_kernel and
    lars_kernel, to which such a launch is no optimizer step - t moves from k to k + 1 with the
    ticket re-armed.  n = 1027: 256 quads, one full block, plus a 3-element tail; n = 1031: 257
    quads, so two blocks (the ticket counts two arrivals), plus a 3-element tail."""
    assert ((n >> 2) + 255) // 256 == (1 if n == 1027 else 2) and n % 4 == 3
    gen = torch.Generator().manual_seed(5)
    p0, m0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    pb, p = guarded(n, torch.float32)
    mb, m = guarded(n, torch.float32)
    sb, sh = guarded(n, torch.bfloat16)
    p.copy_(p0)
    m.copy_(m0)
    g = torch.randn(n, generator=gen).to(dev)
    sc = Sched(RATES)
    for k in range(2):
        sh.fill_(SENT)
        C.sgd(p, g, m, 999.0, 0.9, 0.0, 1e-2, False, False, False, False, [(0, n, sh, 1, 0, 0, 0)], None, sc.arg())
        torch.cuda.synchronize()
        assert torch.equal(p.cpu(), p0) and torch.equal(m.cpu(), m0), "a shadows-only launch updates nothing"
        assert torch.equal(sh.cpu(), p0.to(torch.bfloat16))
        t, ticket, lr_used = sc.read()
        assert (t, ticket) == (k + 1, 0)
        assert lr_used == torch.tensor(RATES, dtype=torch.float32)[k].item()
    assert guards_intact(pb, n) and guards_intact(mb, n) and guards_intact(sb, n)


def test_binding_checks_the_schedule_operands(C):
    p, g = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    table = torch.ones(3, device=dev)
    args = (p, g, None, 0.1, 0.0, 0.0, 0.0, False, False, False, True, [], None)
    for bad in ((table, torch.zeros(2, dtype=torch.int32, device=dev)),          # state too short
                (table, torch.zeros(4, dtype=torch.float32, device=dev)),        # wrong dtype
                (table[:0], torch.zeros(4, dtype=torch.int32, device=dev)),      # empty table
                (table.double(), torch.zeros(4, dtype=torch.int32, device=dev)),
                (table.cpu(), torch.zeros(4, dtype=torch.int32, device=dev))):
        with pytest.raises(RuntimeError):
            C.sgd(*args, bad)
    torch.cuda.synchronize()
    assert not p.any()


# ------------------------------------------------------------------------------ FusedSGD
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


SEVEN = [0.05, 0.2, 0.1, 0.025, 0.15, 0.0125, 0.075]


def test_captured_graph_follows_the_schedule():
    """SimpleCNN's module path at batch 8 in a GraphedStep: 1 warm-up step + 6 replays over a
    7-entry table.  Bitwise the eager run with the same schedule, bitwise NOT the graphed run at
    the constant base rate, and the device counter stands at 7."""
    from ddp_amd.engine import GraphedStep
    from ddp_amd.ops import FusedSGD

    data = _batches(7)

    def run(schedule, graphed):
        model = _simplecnn()
        opt = FusedSGD(model, lr=SEVEN[0], momentum=0.9,
                       lr_schedule=LRSchedule.from_values(SEVEN) if schedule else None)
        step = _step_fn(model, opt)
        if graphed:
            gs = GraphedStep(step, data[0], warmup=1)
            for x, y in data[1:]:
                gs(x, y)
            assert gs.replays == 6
        else:
            for x, y in data:
                step(x, y)
        torch.cuda.synchronize()
        return opt, opt.flat.params.clone(), opt.momentum_buffer.clone()

    og, pg, mg = run(True, True)
    oe, pe, me = run(True, False)
    _, pc, _ = run(False, True)
    assert og.schedule_step() == 7 == oe.schedule_step()
    assert torch.equal(pg, pe) and torch.equal(mg, me), "replays did not follow the eager schedule"
    assert not torch.equal(pg, pc), "the graphed run ignored the schedule"
    table, state = og._sched_ws
    s = state.cpu()
    assert int(s[1]) == 0 and s[2:3].view(torch.float32)[0].item() == table[6].item()
    assert og.current_lr() == table[6].item()  # past the end: the last entry holds
    # an eager step after the replays (the ragged tail of a graphed epoch) continues the sequence
    _step_fn(og.model, og)(*data[0])
    assert og.schedule_step() == 8


def test_fused_sgd_schedule_with_clipping_equals_per_step_by_value_rates():
    """<true, true> through FusedSGD: eager steps with a schedule and max_grad_norm against eager
    steps whose by-value lr is set to the table's entry before each step.  set_schedule_step,
    current_lr and the state dict read the device counter."""
    from ddp_amd.ops import FusedSGD

    data = _batches(4)
    sched = LRSchedule(0.1, 6, "cosine", warmup_steps=2, lr_min=1e-3)
    a, b = _simplecnn(), _simplecnn()
    oa = FusedSGD(a, lr=0.1, momentum=0.9, weight_decay=1e-3, max_grad_norm=0.05, lr_schedule=sched)
    ob = FusedSGD(b, lr=0.1, momentum=0.9, weight_decay=1e-3, max_grad_norm=0.05)
    oa.set_schedule_step(1)  # before the first step: the state block starts from it
    sa, sb = _step_fn(a, oa), _step_fn(b, ob)
    for k, (x, y) in enumerate(data):
        assert oa.schedule_step() == k + 1 and oa.current_lr() == sched.table[min(k + 1, 5)].item()
        ob.param_groups[0]["lr"] = sched.table[min(k + 1, 5)].item()
        sa(x, y)
        sb(x, y)
    assert torch.equal(oa.flat.params, ob.flat.params) and torch.equal(oa.momentum_buffer, ob.momentum_buffer)
    assert oa.grad_clip_stats() == ob.grad_clip_stats() and oa.grad_clip_stats()["clipped"] == 4
    sd = oa.state_dict()
    assert list(sd["param_groups"][0]) == list(ob.state_dict()["param_groups"][0])
    assert sd["param_groups"][0]["lr"] == sched.table[5].item()
    oa.set_schedule_step(2)
    assert oa.schedule_step() == 2 and oa.current_lr() == sched.table[2].item()
    sa(*data[0])
    assert oa.schedule_step() == 3 and int(oa._sched_ws[1][1].item()) == 0


# ------------------------------------------------------------------------------------ CLI
def test_cli_resnet18_graph_module_records_the_scheduled_rate(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    metrics = str(tmp_path / "m.jsonl")
    cmd = [sys.executable, "-u", os.path.join(REPO, "train_ddp.py"), "--world_size", "1", "--device", "gpu",
           "--model", "resnet18", "--image_size", "64", "--num_classes", "10", "--dataset_size", "64",
           "--batch_size", "16", "--graph_module", "--epochs", "2", "--lr_schedule", "cosine", "--warmup_steps", "2",
           "--metrics_json", metrics, "--log_every", "1000", "--checkpoint_dir", str(tmp_path / "ck")]
    p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=240)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    recs = [json.loads(ln) for ln in open(metrics)]
    assert [r["steps"] for r in recs] == [4, 4]  # 64 images / batch 16
    table = LRSchedule(0.01, 8, "cosine", warmup_steps=2).table  # --lr's default, 2 epochs x 4 steps
    assert [r["lr"] for r in recs] == [table[4].item(), table[7].item()]
    assert recs[0]["lr"] != recs[1]["lr"]
    ck = torch.load(tmp_path / "ck" / "epoch_1.pt", weights_only=True)
    assert ck["optimizer"]["param_groups"][0]["lr"] == table[7].item()
