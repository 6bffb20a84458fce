"""The weight EMA on the GPU: ema_kernel<false> / ema_kernel<true> (csrc/kernels/ema.hip) per
element against the float64 reference under the bound derived in tests/test_ema_cpu.py, their
counters, hipGraph replay of a warm-up EMA, ema_swap_kernel with every shadow kind, evaluation
under ``applied()`` against a fresh model holding the averaged weights, and the CLI."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from ddp_amd.ops import CrossEntropyLoss, FusedSGD, WeightEMA
from ddp_amd.ops import kernel_bounds as kb
from ddp_amd.ops.ema import warmup_table
from test_ema_cpu import ema_bound, f32, mixed_inputs

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 64  # guard elements after each buffer
# tail only, one quad, a ragged block, two blocks + tail, the 2048-block cap with a second grid-stride pass
SIZES = [1, 3, 4, 1023, 4 * 256 + 1, 2048 * 256 * 4 + 4 * 300 + 3]
ISENT = 0x5A5A5A5A


def guarded(host):
    """``host`` on the device with a NaN-prefilled guard band after it."""
    n = host.numel()
    buf = torch.full((n + G,), float("nan"), dtype=torch.float32, device=dev)
    buf[:n].copy_(host)
    return buf, buf[:n]


def guard_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


# ------------------------------------------------------------------------------- ema_kernel
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_per_element_over_7_launches(C, n, warm):
    """Seven launches from mixed-sign, mixed-magnitude inputs, the parameters moved between them;
    each launch against the reference of its own inputs.  The warm-up build reads a five-entry
    table: launches 5 and 6 hold its last entry.  The counter is exact, the words around the
    state block, the guard bands and p are untouched."""
    e0 = mixed_inputs(n, n % 1000)
    p_host = (e0.double() * (1 + 1e-3 * torch.randn(n, generator=torch.Generator().manual_seed(n % 1000 + 1),
                                                    dtype=torch.float64))).float()
    ebuf, e = guarded(e0)
    pbuf, p = guarded(p_host)
    table_host = warmup_table(0.9)[:5].contiguous()
    tbuf, table = guarded(table_host)
    sbuf = torch.full((12,), ISENT, dtype=torch.int32, device=dev)
    state = sbuf[4:8]
    state.copy_(torch.tensor([0, 0, 0, 0], dtype=torch.int32))
    om_const = f32(1 - 0.999)
    cur = e0.numpy().copy()
    for k in range(7):
        if k == 2:  # unrelated values
            p_host = mixed_inputs(n, 4242 + n % 1000)
            p.copy_(p_host)
        elif k == 4:
            p_host = -p_host
            p.copy_(p_host)
        om = table_host[min(k, 4)].item() if warm else om_const
        C.ema(e, p, om_const, state, table if warm else None)
        got = e.cpu().numpy()
        ref, bound = ema_bound(cur, p_host.numpy(), om)
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err <= bound), (k, float((err / np.maximum(bound, 1e-300)).max()))
        assert torch.equal(p.cpu(), p_host), "p is read-only"
        cur = got
    s = sbuf.cpu()
    assert bool((s[:4] == ISENT).all()) and bool((s[8:] == ISENT).all()), "words around the state were written"
    assert int(s[4]) == 7, "num_updates after 7 launches"
    assert int(s[5]) == 0 and int(s[7]) == 0
    if warm:
        assert s[6:7].view(torch.float32)[0].item() == table_host[4].item(), "the decay last used"
    else:
        assert int(s[6]) == 0, "the constant-decay build writes the counter alone"
    assert guard_intact(ebuf, n) and guard_intact(pbuf, n) and guard_intact(tbuf, 5)
    assert torch.equal(table.cpu(), table_host), "the table is read-only"


def test_binding_rejects_bad_operands(C):
    n = 64
    e, p = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    table = warmup_table(0.9).to(dev)
    both = torch.zeros(2 * n, device=dev)
    for bad in (lambda: C.ema(e[:60], p, 0.1, state, None),            # sizes differ
                lambda: C.ema(both[1:n + 1], p, 0.1, state, None),      # not 16-byte aligned
                lambda: C.ema(e, p, 0.1, state[:2], None),              # state too short
                lambda: C.ema(e, p, 0.1, state, table.double()),        # table dtype
                lambda: C.ema(e, p, 0.0, state, None),                  # om outside (0, 1)
                lambda: C.ema(e, p, 1.0, state, None),
                lambda: C.ema(p, p, 0.1, state, None),                  # aliased
                lambda: C.ema(both[:n], both[n - 4:2 * n - 4], 0.1, state, None),  # overlapping
                lambda: C.ema(e.cpu(), p, 0.1, state, None),
                lambda: C.ema_swap(p, p, []),
                lambda: C.ema_swap(p, e[:60], []),
                lambda: C.ema_swap(p, e, [(0, n + 4, torch.zeros(n + 4, dtype=torch.bfloat16, device=dev), 1, 0, 0, 0)])):
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()
    assert int(state[0]) == 0 and not e.any() and not p.any(), "a refused call launches nothing"


# ----------------------------------------------------------------------------- graph replay
def _simplecnn():
    from ddp_amd.models import SimpleCNN

    torch.manual_seed(0)
    return SimpleCNN().to(dev)


def _step_fn(model, opt):
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


def test_captured_graph_follows_the_warmup_decay():
    """SimpleCNN's module path at batch 8 with an attached warm-up EMA in a GraphedStep: the
    warm-up step, then 6 replays on different batches.  The EMA buffer and its counter are
    bitwise those of the same steps run eagerly from the same start - a kernel that captured
    ``om`` by value would replay update 1's decay six times."""
    from ddp_amd.engine import GraphedStep

    data = _batches(7)

    def run(graphed):
        model = _simplecnn()
        opt = FusedSGD(model, lr=0.05, momentum=0.9)
        ema = WeightEMA(model, decay=0.99, warmup=True)
        opt.attach_ema(ema)
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
        return ema, ema.params.clone(), opt.flat.params.clone()

    eg, ag, pg = run(True)
    ee, ae, pe = run(False)
    assert eg.num_updates() == 7 == ee.num_updates()
    assert torch.equal(pg, pe) and torch.equal(ag, ae), "the replays did not follow the eager updates"
    assert not torch.equal(ag, pg)
    s = eg._ws[1].cpu()
    assert int(s[1]) == 0 and s[2:3].view(torch.float32)[0].item() == eg.om_at(6)
    assert len({eg.om_at(k) for k in range(7)}) == 7, "seven different decays"
    # an eager step after the replays (the ragged tail of a graphed epoch) continues the sequence
    _step_fn(eg.model, eg._opt)(*data[0])
    assert eg.num_updates() == 8


# ------------------------------------------------------------------------- ema_swap_kernel
def _rebuild(kind, src32, n, a=0, b=0, c=0):
    """The shadow of fp32 ``src32`` (host) the writers of shadow.h produce, rebuilt on the host."""
    idx = torch.from_numpy(kb.shadow_index(kind, n, a, b, c))
    f32k = kb.shadow_is_f32(kind)
    dst = torch.zeros(kb.shadow_dst_numel(kind, n), dtype=torch.float32 if f32k else torch.bfloat16)
    dst[idx] = src32 if f32k else src32.to(torch.bfloat16)  # (.to(bfloat16): round to nearest even)
    return dst


def _check_applied_and_restored(model, opt, ema, shadows_of):
    """``shadows_of()``: [(kind, off, n, a, b, c, device tensor)] of every shadow to check."""
    fs = ema.flat
    torch.cuda.synchronize()
    p0, e0, g0 = fs.params.clone(), ema.params.clone(), fs.grads.clone()
    sh0 = [t.clone() for *_, t in shadows_of()]
    bufs0 = [b.clone() for b in model.buffers()]
    assert not torch.equal(p0, e0)
    with ema.applied():
        torch.cuda.synchronize()
        assert torch.equal(fs.params, e0), "inside, the parameters hold the EMA's bits"
        assert torch.equal(ema.params, p0)
        host = e0.cpu()
        for kind, off, n, a, b, c, t in shadows_of():
            want = _rebuild(kind, host[off:off + n], n, a, b, c)
            assert torch.equal(t.cpu().flatten(), want), f"shadow kind {kind} at {off} is not the EMA's"
        for p in model.parameters():
            assert torch.equal(fs.bf16_view(p), p.detach().to(torch.bfloat16)), "bf16_view is stale inside applied()"
    torch.cuda.synchronize()
    assert torch.equal(fs.params, p0) and torch.equal(ema.params, e0) and torch.equal(fs.grads, g0)
    for (*_, t), want in zip(shadows_of(), sh0):
        assert torch.equal(t, want), "a shadow was not restored"
    for b, want in zip(model.buffers(), bufs0):
        assert torch.equal(b, want)


def test_swap_resnet18_with_the_pad4_copy():
    """ResNet-18 at 64x64: the bf16 copy and the stem's PAD4 copy (materialised by a forward)."""
    from ddp_amd.models import resnet18

    torch.manual_seed(0)
    model = resnet18(num_classes=10).to(dev)
    opt = FusedSGD(model, lr=0.05, momentum=0.9)
    ema = WeightEMA(model, decay=0.5)
    opt.attach_ema(ema)
    g = torch.Generator().manual_seed(3)
    step = _step_fn(model, opt)
    for _ in range(2):
        step(torch.randn(4, 3, 64, 64, generator=g).to(dev), torch.randint(0, 10, (4,), generator=g).to(dev))
    fs = ema.flat
    assert fs._bf16 is not None and len(fs._pad4) == 1, "the forward materialises both copies"

    def shadows_of():
        out = [(kb.SHADOW_BF16, 0, fs.numel, 0, 0, 0, fs._bf16)]
        out += [(kb.SHADOW_BF16_PAD4, off, n, 0, 0, 0, buf) for off, n, buf, *_ in fs.pad4_shadows()]
        return out

    _check_applied_and_restored(model, opt, ema, shadows_of)


def test_swap_simplecnn_with_registered_shadows_and_a_captured_graph():
    """SimpleCNN with the optimizer's registered shadows - conv2's weight transposed in bf16 and
    fp32, the fc weight in fragment order in bf16 - beside the bf16 copy (MAX_SHADOWS = 4).
    Then: a step graph captured before the exchange replays, after it, to the bits of a run that
    never exchanged."""
    from ddp_amd.engine import GraphedStep

    data = _batches(5)

    def run(swap):
        model = _simplecnn()
        opt = FusedSGD(model, lr=0.05, momentum=0.9)
        fs = opt.flat
        fs.bf16_params()  # materialise the bf16 copy (SimpleCNN's module path reads the fp32 weights)
        w2, wfc = model.net[2].weight, model.fl.weight
        o2, n2, ofc, nfc = fs.offsets["net.2.weight"], w2.numel(), fs.offsets["fl.weight"], wfc.numel()
        co, taps, ci = w2.shape[0], w2.shape[1] * w2.shape[2], w2.shape[3]
        hw, ch = wfc.shape[1], wfc.shape[2]
        regs = [(kb.SHADOW_BF16_TAPT, o2, n2, co, taps, ci, torch.zeros(n2, dtype=torch.bfloat16, device=dev)),
                (kb.SHADOW_F32_TAPT, o2, n2, co, taps, ci, torch.zeros(n2, dtype=torch.float32, device=dev)),
                (kb.SHADOW_BF16_FCFRAG, ofc, nfc, hw, ch, 0, torch.zeros(nfc, dtype=torch.bfloat16, device=dev))]
        opt.shadows = [(off, n, t, kind, a, b, c) for kind, off, n, a, b, c, t in regs]
        ema = WeightEMA(model, decay=0.9, warmup=True)
        opt.attach_ema(ema)
        gs = GraphedStep(_step_fn(model, opt), data[0], warmup=1)
        gs(*data[1])
        gs(*data[2])
        if swap:
            _check_applied_and_restored(model, opt, ema, lambda: regs + [(kb.SHADOW_BF16, 0, fs.numel, 0, 0, 0, fs._bf16)])
        gs(*data[3])
        gs(*data[4])
        torch.cuda.synchronize()
        return [fs.params.clone(), ema.params.clone(), opt.momentum_buffer.clone(), fs._bf16.clone(),
                *[t.clone() for *_, t in regs]], ema.num_updates()

    a, ka = run(True)
    b, kb_ = run(False)
    assert ka == kb_ == 5
    for x, y in zip(a, b):
        assert torch.equal(x, y), "the exchange left a trace in the captured graph's replays"


# ------------------------------------------------------------------- evaluation equivalence
def test_evaluate_resnet_under_applied_equals_a_fresh_averaged_model():
    from ddp_amd.data import DeviceImages, synthetic_imagenet_test
    from ddp_amd.engine.evaluation import evaluate_resnet
    from ddp_amd.models import resnet18

    torch.manual_seed(0)
    model = resnet18(num_classes=10).to(dev)
    opt = FusedSGD(model, lr=0.05, momentum=0.9)
    ema = WeightEMA(model, decay=0.5)
    opt.attach_ema(ema)
    g = torch.Generator().manual_seed(5)
    step = _step_fn(model, opt)
    for _ in range(3):
        step(torch.randn(8, 3, 64, 64, generator=g).to(dev), torch.randint(0, 10, (8,), generator=g).to(dev))
    imgs, labels = synthetic_imagenet_test(64, 64, 10, seed=2, n_train=16)
    split = DeviceImages(imgs, labels, dev)
    fresh = resnet18(num_classes=10).to(dev)
    fresh.load_state_dict(ema.state_dict()["model"])
    live = evaluate_resnet(model, split, batch_size=32, want_logits=True)
    with ema.applied():
        avg = evaluate_resnet(model, split, batch_size=32, want_logits=True)
    ref = evaluate_resnet(fresh, split, batch_size=32, want_logits=True)
    again = evaluate_resnet(model, split, batch_size=32, want_logits=True)
    assert avg.count == ref.count == 64
    assert (avg.correct, avg.correct5) == (ref.correct, ref.correct5)
    assert torch.equal(avg.pred, ref.pred) and torch.equal(avg.logits, ref.logits) and torch.equal(avg.loss, ref.loss)
    assert not torch.equal(avg.logits, live.logits), "the averaged model is another model"
    assert torch.equal(again.logits, live.logits) and torch.equal(again.pred, live.pred), "applied() left a trace"


def test_evaluate_simplecnn_fused_under_applied_equals_a_fresh_averaged_model():
    from ddp_amd.data import DeviceMNIST
    from ddp_amd.data.mnist import synthetic_mnist_test
    from ddp_amd.engine.evaluation import evaluate
    from ddp_amd.models import SimpleCNN

    model = _simplecnn()
    opt = FusedSGD(model, lr=0.05, momentum=0.9)
    ema = WeightEMA(model, decay=0.9, warmup=True)
    opt.attach_ema(ema)
    step = _step_fn(model, opt)
    for x, y in _batches(3):
        step(x, y)
    imgs, labels = synthetic_mnist_test(200, n_train=512)
    split = DeviceMNIST(imgs, labels, dev)
    fresh = SimpleCNN().to(dev)
    fresh.load_state_dict(ema.state_dict()["model"])
    live = evaluate(model, split, engine="fused", batch_size=128, want_logits=True)
    with ema.applied():
        avg = evaluate(model, split, engine="fused", batch_size=128, want_logits=True)
    ref = evaluate(fresh, split, engine="fused", batch_size=128, want_logits=True)
    assert avg.count == ref.count == 200 and avg.correct == ref.correct
    assert torch.equal(avg.pred, ref.pred) and torch.equal(avg.logits, ref.logits)
    assert not torch.equal(avg.logits, live.logits)
    again = evaluate(model, split, engine="fused", batch_size=128, want_logits=True)
    assert torch.equal(again.logits, live.logits)


# ------------------------------------------------------------------------------------ CLI
EVAL_LINE = re.compile(r"Epoch (\d+) \| (Eval|Eval EMA) \| Loss: ([\d.]+) \| Accuracy: ([\d.]+)% \((\d+)/(\d+)\) \| "
                       r"Top-5: ([\d.]+)% \((\d+)/(\d+)\)")


def test_cli_resnet18_graph_module_ema(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    metrics = str(tmp_path / "m.jsonl")

    def train(*args):
        cmd = [sys.executable, "-u", os.path.join(REPO, "train_ddp.py"), "--world_size", "1", "--device", "gpu",
               "--model", "resnet18", "--graph_module", "--image_size", "64", "--num_classes", "10",
               "--dataset_size", "64", "--batch_size", "16", "--log_every", "1000", "--epochs", "2",
               "--ema_decay", "0.99", "--ema_warmup", "--eval_size", "64", "--eval_ema",
               "--checkpoint_dir", str(tmp_path / "ck"), *args]
        p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=240)
        assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        return p.stdout

    out = train("--eval_every", "1", "--metrics_json", metrics)
    lines = EVAL_LINE.findall(out)
    assert [(m[0], m[1]) for m in lines] == [("0", "Eval"), ("0", "Eval EMA"), ("1", "Eval"), ("1", "Eval EMA")], out
    for m in lines:
        assert m[5] == "64" == m[8] and 0 <= int(m[4]) <= int(m[7]) <= 64
    ck = torch.load(tmp_path / "ck" / "epoch_1.pt", weights_only=True)
    assert list(ck) == ["epoch", "model", "optimizer", "ema"]
    assert ck["ema"]["num_updates"] == 8  # 2 epochs x 64 / 16 optimizer steps
    assert (ck["ema"]["decay"], ck["ema"]["warmup"]) == (0.99, True)
    recs = [json.loads(ln) for ln in open(metrics)]
    assert [r["ema_updates"] for r in recs] == [4, 8]
    for rec, ev, ema in zip(recs, lines[0::2], lines[1::2]):
        assert rec["eval_accuracy"] == int(ev[4]) / 64 and rec["eval_top5"] == int(ev[7]) / 64
        assert rec["eval_ema_accuracy"] == int(ema[4]) / 64 and rec["eval_ema_top5"] == int(ema[7]) / 64
        assert abs(rec["eval_ema_loss"] - float(ema[2])) < 1e-4
    out2 = train("--eval_only")
    assert "Starting epoch" not in out2
    assert EVAL_LINE.findall(out2) == lines[2:], out2
