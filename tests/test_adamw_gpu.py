"""AdamW on the GPU: adamw_kernel (csrc/kernels/adamw.hip) per element against the float64
reference of its documented sequence under the derived bounds (tests/test_adamw_cpu.py, whose
docstring holds the derivation), its in-launch step counter, the binding's operand checks,
FusedAdamW eagerly, under hipGraph replay and against torch.optim.AdamW, and the CLI."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from ddp_amd.ops import FusedAdamW, LRSchedule
from ddp_amd.ops.adamw import coef_table
from test_adamw_cpu import B1, B2, EPS, LR, check_bounds, make_inputs, ref64, scalars32

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 1234.5   # guard-band fill (exact in bf16 and fp32)
ISENT = 0x5A5A5A5A
G = 64          # guard elements on each side (a multiple of 4: 16-byte alignment kept)
BIG = 4 * 256 * 2048 + 4 * 256 + 3  # the 2048-block grid cap and a second grid-stride pass, n % 4 = 3
SIZES = [3, 4, 7, 1029, BIG]  # tail only, one quad, quad + tail, several blocks, the cap
GSCALE = 0.37


def guarded(n, dtype):
    buf = torch.full((n + 2 * G,), SENT, dtype=dtype, device=dev)
    return buf, buf[G:G + n]


def guards_intact(buf, n):
    return bool((buf[:G] == SENT).all()) and bool((buf[G + n:] == SENT).all())


class Sched:
    """(coef table [n, 4], state) for C.adamw's ``sched``, each inside sentinel words."""

    def __init__(self, table, t=0):
        self.host = table.clone()
        self.n = table.shape[0]
        self.tbuf, flat = guarded(4 * self.n, torch.float32)
        self.table = flat.view(self.n, 4)
        self.table.copy_(table)
        self.sbuf = torch.full((12,), ISENT, dtype=torch.int32, device=dev)
        self.state = self.sbuf[4:8]
        self.state.copy_(torch.tensor([t, 0, 0, 0], dtype=torch.int32))

    def arg(self):
        return (self.table, self.state)

    def read(self):
        s = self.sbuf.cpu()
        assert bool((s[:4] == ISENT).all()) and bool((s[8:] == ISENT).all()), "words around the state were written"
        assert int(s[7]) == 0, "SchedState is three words"
        assert guards_intact(self.tbuf, 4 * self.n) and torch.equal(self.table.cpu(), self.host), "the table is read-only"
        return int(s[4]), int(s[5]), s[6:7].view(torch.float32)[0].item()


@functools.lru_cache(maxsize=None)
def inputs(n):
    return make_inputs(n, seed=n % 1000, nzero=min(1000, n // 4))  # (small n: most gradients non-zero)


@functools.lru_cache(maxsize=None)
def table(wd):
    return coef_table(LR, (B1, B2), wd)[:16].contiguous()


OPTIONS = {  # weight decay, maximize, clip, bf16 shadow
    "wd0": (0.0, False, False, False), "wd": (1e-2, False, False, False), "maximize": (1e-2, True, False, False),
    "clip": (1e-2, False, True, False), "shadow": (1e-2, False, False, True),
}


@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("n", SIZES)
def test_kernel_per_element(C, n, opt):
    wd, maximize, clip, shadow = OPTIONS[opt]
    p0, g0, m0, v0 = inputs(n)
    for t in (0, 1, 9):
        hm, hv = (torch.zeros(n), torch.zeros(n)) if t == 0 else (m0, v0)
        bufs = [guarded(n + (-n) % 4, torch.float32) for _ in range(4)]
        (pb, p), (gb, g), (mb, m), (vb, v) = [(b, w[:n]) for b, w in bufs]
        for w, h in ((p, p0), (g, g0), (m, hm), (v, hv)):
            w.copy_(h)
        for _, w in bufs:
            w[n:] = SENT
        sbuf, sh = guarded(n + (-n) % 4, torch.bfloat16)
        gsb, gs = guarded(4, torch.float32)
        gs.fill_(GSCALE)
        sc = Sched(table(wd), t)
        shadows = [(0, n, sh[:n], 1, 0, 0, 0)] if shadow else []
        C.adamw(p, g, m, v, B1, B2, EPS, maximize, True, shadows, gs[:1] if clip else None, sc.arg())
        torch.cuda.synchronize()
        ref = ref64(p0, g0, hm, hv, scalars32(t + 1, wd=wd), gscale=GSCALE if clip else None, maximize=maximize)
        check_bounds((p.cpu(), m.cpu(), v.cpu()), ref, f"kernel n={n} {opt} t={t}")
        for b, _ in bufs:
            assert bool((b[:G] == SENT).all()) and bool((b[G + n:] == SENT).all()), "guard band written"
        assert torch.equal(g.cpu(), g0), "the gradient is read-only"
        assert guards_intact(gsb, 4) and bool((gs == GSCALE).all()), "gscale is read-only"
        if shadow:
            assert torch.equal(sh[:n], p.to(torch.bfloat16)), "shadow != bf16(p)"
            assert bool((sbuf[:G] == SENT).all()) and bool((sbuf[G + n:] == SENT).all())
        else:
            assert bool((sbuf == SENT).all())
        tt, ticket, lr_used = sc.read()
        assert (tt, ticket) == (t + 1, 0) and lr_used == table(wd)[t, 3].item()


@pytest.mark.parametrize("n", [7, 1029])
def test_update_false_rewrites_shadows_only(C, n):
    p0, g0, m0, v0 = inputs(n)
    p, g, m, v = (x.to(dev) for x in (p0, g0, m0, v0))
    sbuf, sh = guarded(n + (-n) % 4, torch.bfloat16)
    sc = Sched(table(1e-2), 5)
    C.adamw(p, g, m, v, B1, B2, EPS, False, False, [(0, n, sh[:n], 1, 0, 0, 0)], None, sc.arg())
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0) and torch.equal(m.cpu(), m0) and torch.equal(v.cpu(), v0)
    assert torch.equal(sh[:n], p.to(torch.bfloat16))
    assert bool((sbuf[:G] == SENT).all()) and bool((sbuf[G + n:] == SENT).all())
    assert sc.read()[:2] == (5, 0), "a shadows-only launch is no optimizer step"


@pytest.mark.parametrize("n", [7, 4117])
def test_counter_over_300_launches(C, n):
    """One block and several: after 300 launches t == 300, the ticket is re-armed, lr_used is
    the last entry, and a three-entry table is held at its last entry from launch 3 on."""
    three = coef_table(LR, (B1, B2), 1e-2)[:3].contiguous()
    three[:, 3] = torch.tensor([0.25, 0.5, 0.75])
    p0, g0, _, _ = inputs(n)

    def run(tab, launches, state_t=0):
        p, g = p0.to(dev), g0.to(dev)
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        sc = Sched(tab, state_t)
        for _ in range(launches):
            C.adamw(p, g, m, v, B1, B2, EPS, False, True, [], None, sc.arg())
        torch.cuda.synchronize()
        return p, m, v, sc

    p, m, v, sc = run(three, 300)
    assert sc.read() == (300, 0, 0.75)
    # launches 3.. use entry 2: the same bits as a one-entry table of entry 2 from launch 3 on
    pa, ma, va, sa = run(three, 3)
    assert sa.read() == (3, 0, 0.75)
    sb = Sched(three[2:3].contiguous(), 0)
    gd = g0.to(dev)
    for _ in range(297):
        C.adamw(pa, gd, ma, va, B1, B2, EPS, False, True, [], None, sb.arg())
    torch.cuda.synchronize()
    assert sb.read() == (297, 0, 0.75)
    assert torch.equal(p, pa) and torch.equal(m, ma) and torch.equal(v, va)


def test_binding_rejects_bad_operands(C):
    n = 1029
    mk = lambda: [torch.zeros(n, device=dev) for _ in range(4)]  # noqa: E731
    p, g, m, v = mk()
    tab = table(1e-2).to(dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    args = lambda p=p, g=g, m=m, v=v: (p, g, m, v, B1, B2, EPS, False, True, [], None)  # noqa: E731
    off = torch.zeros(n + 1, device=dev)[1:]  # 4-byte aligned only
    bad = [
        (args(), None),                                                  # sched is required
        (args(), (tab, state[:2])),                                      # short state
        (args(), (tab, state.float())),                                  # state dtype
        (args(), (tab.double(), state)),                                 # table dtype
        (args(), (tab[:0], state)),                                      # empty table
        (args(), (tab.flatten()[:6], state)),                            # ragged table
        (args(), (tab[:, :2], state)),                                   # non-contiguous table
        (args(), (tab.cpu(), state)),                                    # CPU table
        (args(m=off), (tab, state)), (args(v=off), (tab, state)),        # misaligned moments
        (args(m=m[:8]), (tab, state)),                                   # moment size
        (args(v=v.double()), (tab, state)), (args(g=g.half()), (tab, state)),  # dtypes
    ]
    for a, s in bad:
        with pytest.raises((RuntimeError, TypeError)):
            C.adamw(*a, s)
    with pytest.raises((RuntimeError, TypeError)):
        C.adamw(p, g, m, v, B1, B2, EPS, False, True, [(0, n + 1, torch.zeros(n + 1, dtype=torch.bfloat16, device=dev),
                                                        1, 0, 0, 0)], None, (tab, state))
    torch.cuda.synchronize()
    assert not p.any() and not m.any() and not v.any() and not state.any(), "a rejected call wrote something"


def test_kernel_is_deterministic(C):
    n = BIG
    p0, g0, m0, v0 = inputs(n)
    outs = []
    for _ in range(2):
        p, g, m, v = (x.to(dev) for x in (p0, g0, m0, v0))
        sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        gs = torch.full((1,), GSCALE, device=dev)
        sc = Sched(table(1e-2), 3)
        C.adamw(p, g, m, v, B1, B2, EPS, False, True, [(0, n, sh, 1, 0, 0, 0)], gs, sc.arg())
        torch.cuda.synchronize()
        outs.append((p, m, v, sh))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------ FusedAdamW
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


SEVEN = [0.004, 0.016, 0.008, 0.002, 0.012, 0.001, 0.006]


@pytest.mark.parametrize("extras", [False, True])
def test_captured_graph_follows_bias_correction(extras):
    """SimpleCNN's module path at batch 8 in a GraphedStep: 1 warm-up step + 6 replays.
    Parameters and both moments are bitwise those of 7 eager steps and the device counter
    stands at 7 on both - a replay that baked t at capture cannot pass.  ``extras``: the same
    with max_grad_norm and a 7-entry schedule."""
    from ddp_amd.engine import GraphedStep

    data = _batches(7)
    kw = dict(max_grad_norm=0.05, lr_schedule=LRSchedule.from_values(SEVEN)) if extras else {}

    def run(graphed):
        model = _simplecnn()
        opt = FusedAdamW(model, lr=SEVEN[0], **kw)
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
        return opt, opt.flat.params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()

    og, pg, mg, vg = run(True)
    oe, pe, me, ve = run(False)
    assert og.schedule_step() == 7 == oe.schedule_step()
    assert torch.equal(pg, pe) and torch.equal(mg, me) and torch.equal(vg, ve), "replays did not follow the eager steps"
    assert float(og.state_dict()["state"][0]["step"]) == 7.0
    tab, state = og._sched_ws
    s = state.cpu()
    assert int(s[1]) == 0 and s[2:3].view(torch.float32)[0].item() == tab[6, 3].item()
    if extras:
        assert og.current_lr() == torch.tensor(SEVEN[6], dtype=torch.float32).item()  # past the end: the last entry
        assert og.grad_clip_stats() == oe.grad_clip_stats() and og.grad_clip_stats()["steps"] == 7
    # an eager step after the replays (the ragged tail of a graphed epoch) continues the sequence
    _step_fn(og.model, og)(*data[0])
    assert og.schedule_step() == 8


def test_one_gpu_step_against_torch_adamw():
    """From a loaded torch.optim.AdamW state dict (3 torch steps in) and a generated flat
    gradient: our fourth step against torch's, per element under the bound."""
    from ddp_amd.models import reference_simple_cnn

    model = _simplecnn()
    ref = reference_simple_cnn()
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    topt = torch.optim.AdamW(ref.parameters(), lr=LR, weight_decay=1e-2)
    gen = torch.Generator().manual_seed(5)

    def fill_grads():
        for q in ref.parameters():
            q.grad = torch.randn(q.shape, generator=gen) * 10.0 ** (torch.rand(q.shape, generator=gen) * 6 - 5)

    for _ in range(3):
        fill_grads()
        topt.step()
    model.load_state_dict({k: v.to(dev) for k, v in ref.state_dict().items()})
    opt = FusedAdamW(model, lr=LR, weight_decay=1e-2)
    opt.load_state_dict(topt.state_dict())
    assert opt.schedule_step() == 3
    fs = opt.flat
    before = {k: (q.detach().clone(), topt.state[q]["exp_avg"].clone(), topt.state[q]["exp_avg_sq"].clone())
              for k, q in ref.named_parameters()}
    fill_grads()
    fs.reattach_grads()
    grads = {k: q.grad.clone() for k, q in ref.named_parameters()}
    tmp = torch.zeros_like(fs.grads)
    from ddp_amd.ops.flat_optim import _from_reference_layout

    _from_reference_layout(model, fs, {k: v.to(dev) for k, v in grads.items()}, tmp)
    fs.grads.copy_(tmp)
    opt.step()
    topt.step()
    torch.cuda.synchronize()
    assert opt.schedule_step() == 4
    ours_p = {k: v.cpu() for k, v in model.state_dict().items()}
    sd = opt.state_dict()["state"]
    s = scalars32(4)
    for i, (k, q) in enumerate(ref.named_parameters()):
        p0, m0, v0 = before[k]
        r = ref64(p0.flatten(), grads[k].flatten(), m0.flatten(), v0.flatten(), s)
        check_bounds((ours_p[k].flatten(), sd[i]["exp_avg"].cpu().flatten(), sd[i]["exp_avg_sq"].cpu().flatten()),
                     r, f"gpu step 4 {k}")
        assert (ours_p[k].flatten().double() - q.detach().flatten().double()).abs().le(2 * r[3][0]).all(), k


# ------------------------------------------------------------------------------------ CLI
def _cli(args, cwd, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, "-u", os.path.join(REPO, "train_ddp.py"), "--world_size", "1", "--device", "gpu",
           "--optimizer", "adamw", "--log_every", "1", *args]
    p = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return p.stdout


def test_cli_resnet18_graph_module_adamw(tmp_path):
    out = _cli(["--model", "resnet18", "--image_size", "64", "--num_classes", "10", "--dataset_size", "64",
                "--batch_size", "16", "--graph_module", "--epochs", "2", "--lr_schedule", "cosine",
                "--warmup_steps", "2", "--checkpoint_dir", str(tmp_path / "ck")], tmp_path)
    losses = [float(ln.rsplit("Loss:", 1)[1]) for ln in out.splitlines() if "| Loss:" in ln]
    assert len(losses) >= 2 and bool(torch.isfinite(torch.tensor(losses)).all())
    ck = torch.load(tmp_path / "ck" / "epoch_1.pt", weights_only=True)
    osd = ck["optimizer"]
    from ddp_amd.models import resnet18

    params = [torch.nn.Parameter(torch.zeros_like(s["exp_avg"])) for s in osd["state"].values()]
    assert len(params) == len(list(resnet18(num_classes=10).parameters()))
    topt = torch.optim.AdamW(params)
    topt.load_state_dict(osd)
    assert float(topt.state[params[0]]["step"]) == 8.0 == float(osd["state"][0]["step"])
    sched = LRSchedule(0.01, 8, "cosine", warmup_steps=2)  # --lr's default, 2 epochs x 4 steps
    assert osd["param_groups"][0]["lr"] == sched.table[7].item()  # step 8's rate: the last entry holds


def test_cli_resume_is_bitwise_the_uninterrupted_run(tmp_path):
    common = ["--engine", "module", "--max_steps", "6", "--batch_size", "32", "--data", "synthetic",
              "--weight_decay", "0.01", "--lr", "0.001"]
    _cli([*common, "--epochs", "2", "--checkpoint_dir", str(tmp_path / "a")], tmp_path)
    _cli([*common, "--epochs", "1", "--checkpoint_dir", str(tmp_path / "b")], tmp_path)
    out = _cli([*common, "--epochs", "2", "--checkpoint_dir", str(tmp_path / "b")], tmp_path)
    assert "starting at epoch 1" in out and "WARNING" not in out
    a = torch.load(tmp_path / "a" / "epoch_1.pt", weights_only=True)
    b = torch.load(tmp_path / "b" / "epoch_1.pt", weights_only=True)
    assert all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    assert a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"]
    for i, s in a["optimizer"]["state"].items():
        assert float(s["step"]) == 12.0
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(s[k], b["optimizer"]["state"][i][k]), (i, k)
