"""LAMB on the GPU: lamb_moments_kernel per element and per tensor, lamb_apply_kernel per element
(shadows included) against kernel_bounds.lamb_reference under its derived bounds, the FusedLAMB
step eager and as a captured graph, the bindings' operand checks and the CLI."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ddp_amd.ops import FusedLAMB
from ddp_amd.ops import kernel_bounds as kb
from ddp_amd.ops.lamb import lamb_coef_table
from elementwise import bits
from lars_cases import COEF, ITEM, WIDE, Layout
from test_lamb_cpu import check_step
from test_lars_gpu import _batches, _simplecnn  # the module and batches of its SGD anchor

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B1, B2, EPS, LR = 0.9, 0.95, 1e-6, 0.05
# every n % 4, one item exactly, one item +- 1, two items + 3, and 65 items + 1 (the finish's lane
# loop takes a second trip); tensors 1 and 5 excluded (wd 0, phi 1), tensor 2 adapted without decay
EDGES = Layout("edges", [1, 5, 64, 4095, ITEM, ITEM + 1, 2 * ITEM + 3, 65 * ITEM + 1],
               excluded=[False, True, False, False, False, True, False, False])
EDGES.wds[2] = 0.0
LAYOUTS = {"edges": EDGES, "wide": WIDE}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(w, g, m, v) float32 on the host, zero padding; v >= 0 at the gradient's scale squared."""
    w, g, m = LAYOUTS[name].inputs()
    return w, g, m, (m * 20).square()


def nan_padding(L, x):
    """x on the device with NaN in the padding, outside the partial quad an item may touch."""
    out = x.clone()
    for i, (b, n) in enumerate(L.segs):
        out[b + (n + 3) // 4 * 4:L.begins[i + 1] if i + 1 < L.n_seg else L.n] = float("nan")
    return out.to(dev)


class Workspace:
    def __init__(self, C, L, like, t):
        self.plan = C.lars_plan(*L.tables(), L.n, like)
        self.partials = torch.zeros(2 * L.n_items, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sums = torch.zeros(L.n_seg, 2, device=dev)
        self.trust = torch.zeros(L.n_seg + 1, 4, device=dev)
        self.trust[L.n_seg, 0] = 1.0
        self.table = lamb_coef_table(LR, (B1, B2))
        self.sched = (self.table.to(dev), torch.tensor([t, 0, 0, 0], dtype=torch.int32, device=dev))
        self.ibc1, self.bc2, self.lr, _ = self.table[t].tolist()

    def moments(self, C, w, g, m, v, gs=None, **kw):
        C.lamb_moments(w, g, m, v, B1, B2, EPS, False, kw.get("plan", self.plan),
                       self.partials, self.ticket, self.sums, kw.get("trust", self.trust), gs, kw.get("sched", self.sched))

    def apply(self, C, w, m, v, shadows=(), update=True, **kw):
        C.lamb(w, m, v, EPS, update, list(shadows), kw.get("plan", self.plan),
               kw.get("trust", self.trust), kw.get("sched", self.sched))


def within(got, ref, bound, mask, what):
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)[mask]
    assert np.isfinite(err).all() and (err <= bound[mask]).all(), f"{what}: worst error / bound {np.nanmax(err / (bound[mask] + 1e-300))}"


@pytest.mark.parametrize("t", [0, 5])
@pytest.mark.parametrize("clip", [False, True])
def test_moments_pass_per_element_and_per_tensor(C, clip, t):
    L = EDGES
    host = inputs("edges")
    w, g, m, v = (nan_padding(L, x) for x in host)
    before = [bits(x) for x in (w, g, m, v)]
    ws = Workspace(C, L, w, t)
    gs = torch.full((1,), COEF, device=dev) if clip else None
    ws.moments(C, w, g, m, v, gs)
    torch.cuda.synchronize()
    ref = kb.lamb_reference(*(x.numpy() for x in host), L.segs, L.wds, L.adapts, ws.lr, B1, B2, EPS, ws.ibc1, ws.bc2,
                            coef=COEF if clip else None)
    within(m, ref["m"], ref["bm"], L.inside, "m'")
    within(v, ref["v"], ref["bv"], L.inside, "v'")
    for x, b in zip((w, g, m, v), before):  # w and g read-only; every element outside a tensor keeps its bits
        keep = torch.from_numpy(~L.inside) if x is m or x is v else slice(None)
        assert torch.equal(bits(x)[keep], b[keep]), "padding / read-only operand written"
    sums, trust = ws.sums.cpu().numpy(), ws.trust.cpu().numpy()
    assert np.array_equal(sums[:, 0].view(np.int32), L.replay(host[0].numpy())[1].view(np.int32)), "S_w"
    assert np.array_equal(trust[:-1, 2], np.sqrt(sums[:, 0].astype(np.float64)).astype(np.float32)), "|w|"
    assert np.array_equal(trust[:-1, 3], np.sqrt(sums[:, 1].astype(np.float64)).astype(np.float32)), "|u|"
    assert np.array_equal(trust[:-1, 1], np.array(L.wds, np.float32)) and trust[-1].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert (np.abs(trust[:-1, 3] - ref["un"]) <= ref["rel_un"] * ref["un"]).all(), "|u| against float64"
    assert (np.abs(trust[:-1, 0] - ref["phi"]) <= ref["rel_phi"] * ref["phi"]).all(), "phi against float64"
    assert all(trust[i, 0] == 1.0 for i in range(L.n_seg) if not L.adapts[i]) and len(set(trust[:-1, 0])) > 4
    assert ws.sched[1].tolist() == [t, 0, 0, 0] and int(ws.ticket) == 0, "pass 1 advances no counter; its ticket re-arms"
    first = [bits(x).clone() for x in (m, v, ws.sums, ws.trust)]
    m.copy_(nan_padding(L, host[2]))
    v.copy_(nan_padding(L, host[3]))
    ws.moments(C, w, g, m, v, gs)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), f) for x, f in zip((m, v, ws.sums, ws.trust), first)), "a second run differs"


@pytest.mark.parametrize("name", ["edges", "wide"])
def test_apply_pass_per_element_with_shadows(C, name):
    """w' against float64 given the device's own trust table; a plain bf16 shadow over the buffer and
    a PAD4 shadow over the 4095-element tensor through shadow_index; then a shadows-only launch.
    "wide": n_items > 2048 and a second grid-stride pass of flat_stream."""
    L = LAYOUTS[name]
    host = inputs(name)
    w, g, m, v = (x.to(dev) for x in host)
    ws = Workspace(C, L, w, 5)
    ws.moments(C, w, g, m, v)
    plain = torch.full((L.n,), 7.0, dtype=torch.bfloat16, device=dev)
    shadows = [(0, L.n, plain, kb.SHADOW_BF16, 0, 0, 0)]
    if name == "edges":
        b4, n4 = L.segs[3]
        pad = torch.full((kb.shadow_dst_numel(kb.SHADOW_BF16_PAD4, n4),), 7.0, dtype=torch.bfloat16, device=dev)
        shadows.append((b4, n4, pad, kb.SHADOW_BF16_PAD4, 0, 0, 0))
    mv = [bits(m), bits(v), bits(ws.trust)]
    ws.apply(C, w, m, v, shadows)
    torch.cuda.synchronize()
    trust = ws.trust.cpu().numpy()
    ref = kb.lamb_reference(*(x.numpy() for x in host), L.segs, L.wds, L.adapts, ws.lr, B1, B2, EPS, ws.ibc1, ws.bc2,
                            phis=trust[:-1, 0])
    within(w, ref["p"], ref["bp"], L.inside, "w'")
    assert bool((w.cpu()[torch.from_numpy(~L.inside)] == 0).all()), "zero padding stays zero"
    assert [torch.equal(bits(x), b) for x, b in zip((m, v, ws.trust), mv)] == [True] * 3, "pass 2 only reads them"
    assert ws.sched[1].tolist()[:2] == [6, 0] and ws.sched[1][2:3].view(torch.float32).item() == ws.lr
    wb = w.to(torch.bfloat16)
    assert torch.equal(plain, wb), "bf16 shadow"
    if name == "edges":
        idx = torch.from_numpy(kb.shadow_index(kb.SHADOW_BF16_PAD4, n4)).to(dev)
        assert torch.equal(pad[idx], wb[b4:b4 + n4]) and int((pad == 7.0).sum()) == n4 // 3, "PAD4 shadow"
    w_after = bits(w)
    plain.fill_(7.0)
    ws.apply(C, w, m, v, shadows[:1], update=False)
    torch.cuda.synchronize()
    assert torch.equal(bits(w), w_after) and torch.equal(plain, wb) and ws.sched[1].tolist()[:2] == [6, 0]


# ------------------------------------------------------------------------------ FusedLAMB
@pytest.mark.parametrize("clip", [None, 0.05])
def test_fused_lamb_three_steps_eager_and_graphed(clip):
    """Each of three eager steps against the float64 rule from the state before it (bias correction
    moves); 1 warm-up + 2 replays of a captured graph are bitwise those steps."""
    from ddp_amd.engine import GraphedStep
    from ddp_amd.ops import CrossEntropyLoss

    data = _batches(3)

    def make():
        model = _simplecnn()
        opt = FusedLAMB(model, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0.1, max_grad_norm=clip)
        lossf = CrossEntropyLoss()

        def step(x, y, check=None):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            if check is not None:
                opt._prepare_grads()
                before = [t.cpu().numpy().copy() for t in (opt.flat.params.detach(), opt.flat.grads)]
            opt.step()
            if check is not None:
                check(opt, *before)
            return loss
        return opt, step

    opt, step = make()
    fs = opt.flat
    state = {"k": 0, "mv": [np.zeros(fs.numel, np.float32)] * 2}

    def check(opt, w0, g0):
        check_step(opt, state["k"], w0, g0, *state["mv"], EPS, clip, False)
        state.update(k=state["k"] + 1, mv=[opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()])

    for x, y in data:
        step(x, y, check)
    assert opt.schedule_step() == 3 and len({v["ratio"] for v in opt.trust_stats().values()}) > 2
    gopt, gstep = make()
    gs = GraphedStep(gstep, data[0], warmup=1)
    for x, y in data[1:]:
        gs(x, y)
    torch.cuda.synchronize()
    assert gs.replays == 2 and gopt.schedule_step() == 3
    for a, b in ((gopt.flat.params, fs.params), (gopt.exp_avg, opt.exp_avg), (gopt.exp_avg_sq, opt.exp_avg_sq)):
        assert torch.equal(bits(a), bits(b)), "replays did not follow the eager steps"
    assert gopt.trust_stats() == opt.trust_stats()


def test_bindings_refuse_wrong_operands(C):
    L = EDGES
    host = inputs("edges")
    w, g, m, v = (x.to(dev) for x in host)
    ws = Workspace(C, L, w, 0)
    big = torch.zeros(L.n + 4, device=dev)
    for call in (lambda **kw: ws.moments(C, kw.pop("w", w), kw.pop("g", g), kw.pop("m", m), kw.pop("v", v), **kw),
                 lambda **kw: (kw.pop("g", None), ws.apply(C, kw.pop("w", w), kw.pop("m", m), kw.pop("v", v), **kw))):
        with pytest.raises(RuntimeError, match="required"):
            call(m=None)
        with pytest.raises(RuntimeError, match="dtype"):
            call(v=v.double())
        with pytest.raises(RuntimeError, match="GPU tensor"):
            call(m=host[2].clone())
        with pytest.raises(RuntimeError, match="size mismatch"):
            call(v=v[:L.n - 4])
        with pytest.raises(RuntimeError, match="required"):
            call(plan=None)
        with pytest.raises(RuntimeError, match="built for a flat buffer"):
            call(w=big, g=big, m=big, v=big)
        with pytest.raises(RuntimeError, match="trust"):
            call(trust=ws.trust[:L.n_seg])
        with pytest.raises(RuntimeError, match="sched"):
            call(sched=None)
    torch.cuda.synchronize()
    assert all(torch.equal(a.cpu(), b) for a, b in zip((w, g, m, v), host)), "a refused call launched nothing"


# ------------------------------------------------------------------------------------ CLI
def _cli(args, cwd, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, "-u", os.path.join(REPO, "train_ddp.py"), "--world_size", "1", "--device", "gpu",
           "--optimizer", "lamb", "--log_every", "1", "--model", "resnet18", "--image_size", "64", "--num_classes", "10",
           "--dataset_size", "64", "--batch_size", "16", "--graph_module", "--lr", "0.01", "--weight_decay", "0.01",
           "--clip_grad_norm", "5", *args]
    p = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return p.stdout


def test_cli_resnet18_graph_module_lamb_and_bitwise_resume(tmp_path):
    mj = tmp_path / "metrics.jsonl"
    out = _cli(["--epochs", "2", "--metrics_json", str(mj), "--checkpoint_dir", str(tmp_path / "a")], tmp_path)
    losses = [float(ln.rsplit("Loss:", 1)[1]) for ln in out.splitlines() if "| Loss:" in ln]
    assert len(losses) == 8 and bool(torch.isfinite(torch.tensor(losses)).all())
    recs = [json.loads(ln) for ln in mj.read_text().splitlines()]
    assert len(recs) == 2
    for r in recs:
        assert 0 < r["trust_ratio_min"] < r["trust_ratio_max"]
    _cli(["--epochs", "1", "--checkpoint_dir", str(tmp_path / "b")], tmp_path)
    out = _cli(["--epochs", "2", "--checkpoint_dir", str(tmp_path / "b")], tmp_path)
    assert "starting at epoch 1" in out and "WARNING" not in out
    a = torch.load(tmp_path / "a" / "epoch_1.pt", weights_only=True)
    b = torch.load(tmp_path / "b" / "epoch_1.pt", weights_only=True)
    assert all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    assert a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"]
    assert a["optimizer"]["param_groups"][0]["exclude"] == "1d"
    for i, s in a["optimizer"]["state"].items():
        assert float(s["step"]) == 8.0
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(s[k], b["optimizer"]["state"][i][k]), (i, k)
