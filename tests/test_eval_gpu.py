"""The fused inference kernel (csrc/kernels/infer.hip) and the evaluation paths built on it.

Shapes: a 64-image split evaluated in batches of B in {1, 3, 5, 33} - B = 1: 784 pixels leave
the last block partly filled; 3 and 5: blocks straddle two images (784 is no multiple of 64 or
128); 33: more images than one finisher wave's two slots, and a ragged last batch (33 + 31).
Every kernel instantiation (pxt 1 / 2, bf16 / fp32), with and without an index list.  The
oracles run once per module on the CPU (ops/reference.py: the bf16 rounding model in fp32, and
float64 for the exact-fp32 kernel)."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ddp_amd.ops import reference as R

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64
EVAL_LINE = re.compile(r"^Epoch (\d+) \| Eval \| Loss: (\d+\.\d{4}) \| Accuracy: (\d+\.\d{2})% \((\d+)/(\d+)\)$", re.M)


def _native(model):
    return {"w1": model.net[0].weight.detach().cpu(), "b1": model.net[0].bias.detach().cpu(),
            "w2": model.net[2].weight.detach().cpu(), "b2": model.net[2].bias.detach().cpu(),
            "wfc": model.fl.weight.detach().cpu(), "bfc": model.fl.bias.detach().cpu()}


def _oracle_logits(p, x, dtype):
    """x float [n,28,28] in [0,1] -> logits: bf16 = the fp32 model rounding where the kernel
    rounds (a1, a2 and both MFMA weight operands); fp32 = float64."""
    if dtype == "bf16":
        a1 = R.bf16r(R.conv1_relu(x.float(), p["w1"], p["b1"]))
        a2 = R.bf16r(R.conv3x3(a1, R.bf16r(p["w2"]), p["b2"], relu=True))
        return R.fc_nhwc(a2, R.bf16r(p["wfc"]), p["bfc"])
    q = {k: v.double() for k, v in p.items()}
    return R.fc_nhwc(R.conv3x3(R.conv1_relu(x.double(), q["w1"], q["b1"]), q["w2"], q["b2"], relu=True),
                     q["wfc"], q["bfc"])


@pytest.fixture(scope="module")
def setup(C):
    """One model, one 64-image split, the permutation used as the index list, and both oracles
    (per dataset row) - computed once, never modified."""
    from ddp_amd.data import DeviceMNIST
    from ddp_amd.data.mnist import synthetic_mnist_test
    from ddp_amd.engine.evaluation import model_operands
    from ddp_amd.models import SimpleCNN

    torch.manual_seed(11)
    model = SimpleCNN().to(dev)
    imgs, labels = synthetic_mnist_test(N, n_train=N)
    data = DeviceMNIST(imgs, labels, dev)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    p = _native(model)
    x = imgs.float() / 255.0
    return dict(model=model, data=data, labels=labels, perm=perm,
                ops={d: model_operands(model, d) for d in ("bf16", "fp32")},
                ref={d: _oracle_logits(p, x, d) for d in ("bf16", "fp32")})


def _seq_sum(vals):
    s = 0.0
    for v in vals:  # fp64, index order
        s += v
    return s


def _check_outputs(res, labels, ref, dtype):
    lg = res.logits.cpu()
    err = (lg.double() - ref.double()).abs().max().item()
    rel = ((lg.double() - ref.double()).norm() / ref.double().norm()).item()
    print(f"logits: max abs err {err:.3e}, relative (norm) {rel:.3e}, max |logit| {ref.abs().max().item():.3e}")
    if dtype == "bf16":  # test_kernels_gpu.py test_conv3x3_fwd_fused_fc
        torch.testing.assert_close(lg, ref.float(), rtol=1e-3, atol=1e-3)
    else:                # test_fp32_gpu.py
        assert rel < 1e-5
    from ddp_amd.engine.evaluation import lowest_argmax

    pred = res.pred.cpu().long()
    assert torch.equal(pred, lowest_argmax(lg))
    want_loss = torch.logsumexp(lg.double(), dim=1) - lg.double().gather(1, labels.view(-1, 1))[:, 0]
    loss = res.loss.cpu()
    print(f"loss rows: max abs err {(loss.double() - want_loss).abs().max().item():.3e}")
    torch.testing.assert_close(loss.double(), want_loss, rtol=1e-6, atol=1e-6)
    rows = res.correct_rows.cpu()
    assert torch.equal(rows.bool(), pred == labels)
    assert res.count == labels.numel() and res.correct == int(rows.sum())
    assert res.loss_sum == _seq_sum(loss.double().tolist())


@pytest.mark.parametrize("use_idx", [False, True], ids=["rows", "idx"])
@pytest.mark.parametrize("B", [1, 3, 5, 33])
@pytest.mark.parametrize("pxt", [1, 2])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_infer_kernel_outputs(setup, dtype, pxt, B, use_idx):
    from ddp_amd.engine.evaluation import FusedEvaluator

    idx = setup["perm"] if use_idx else None
    res = FusedEvaluator(dev, dtype, pxt).run(setup["data"], setup["ops"][dtype], B, idx, want_logits=True)
    order = setup["perm"] if use_idx else torch.arange(N)
    _check_outputs(res, setup["labels"][order], setup["ref"][dtype][order], dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_tie_rule_lowest_index(setup, dtype):
    """fc weight and bias zero: every logit is 0, every prediction class 0, every loss ln 10."""
    from ddp_amd.engine.evaluation import FusedEvaluator

    ops = dict(setup["ops"][dtype])
    ops["wfc_frag"] = torch.zeros_like(ops["wfc_frag"])
    ops["bfc"] = torch.zeros_like(ops["bfc"])
    for pxt in (1, 2):
        res = FusedEvaluator(dev, dtype, pxt).run(setup["data"], ops, 5, None, want_logits=True)
        assert res.pred.cpu().tolist() == [0] * N
        assert (res.loss.cpu().double() - math.log(10.0)).abs().max().item() <= 1e-6
        assert res.correct == int((setup["labels"] == 0).sum())


def _engine(dtype, B, n_train=512, momentum=0.0, graph=False, graph_steps=5, seed=0):
    from ddp_amd.data import DeviceMNIST, synthetic_mnist
    from ddp_amd.engine import EngineOptions, FusedSimpleCNNEngine
    from ddp_amd.models import SimpleCNN
    from ddp_amd.ops import FusedSGD

    torch.manual_seed(seed)
    model = SimpleCNN(compute_dtype=torch.float32 if dtype == "fp32" else torch.bfloat16).to(dev)
    opt = FusedSGD(model, lr=0.01, momentum=momentum)
    imgs, labels = synthetic_mnist(n_train)
    data = DeviceMNIST(imgs, labels, dev)
    eng = FusedSimpleCNNEngine(model, opt, data, B, 1, 0,
                               opts=EngineOptions(use_graph=graph, graph_steps=graph_steps, dtype=dtype))
    eng.refresh()
    return eng, data


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_eval_loss_is_the_training_forwards_loss_bit_for_bit(C, dtype):
    """The level-3 training forward writes each image's loss (loss_rows); the inference kernel
    run on the same images at the same pxt gives the same bits."""
    eng, data = _engine(dtype, 8)
    if not eng.level3:
        pytest.skip("the level-3 forward is not active at B = 8 on this device")
    eng.sampler.set_epoch(0)
    idx = eng.sampler.indices()[:8]  # what step 0 consumes
    res = eng.evaluate(data, 8, idx, pxt=eng.opts.pxt_fwd)
    eng.run_steps(1)
    eng.synchronize()
    assert torch.equal(res.loss.cpu(), eng.t["loss_rows"][:8].cpu())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_scratch_rearms(setup, dtype):
    """The tickets are left at zero: the same call twice, then another batch size, on one
    evaluator's scratch give what fresh scratch gives."""
    from ddp_amd.engine.evaluation import FusedEvaluator

    ev = FusedEvaluator(dev, dtype, 2)
    runs = [ev.run(setup["data"], setup["ops"][dtype], B, setup["perm"], want_logits=True) for B in (33, 33, 5)]
    fresh = FusedEvaluator(dev, dtype, 2).run(setup["data"], setup["ops"][dtype], 5, setup["perm"], want_logits=True)
    for a, b in ((runs[0], runs[1]), (runs[2], fresh)):
        assert (a.correct, a.count, a.loss_sum) == (b.correct, b.count, b.loss_sum)
        for k in ("pred", "loss", "logits", "correct_rows"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not ev.img_cnt.any().item()


def test_evaluate_does_not_disturb_training(setup):
    """200 images, B = 8, 2 epochs of graph replays: with an evaluation after each epoch and
    without, parameters, momentum and the loss history are bitwise equal."""
    out = []
    for with_eval in (True, False):
        eng, _ = _engine("bf16", 8, n_train=200, momentum=0.9, graph=True, graph_steps=5)
        for epoch in range(2):
            eng.run_epoch(epoch)
            if with_eval:
                res = eng.evaluate(setup["data"], 33)
                assert res.count == N and 0 <= res.correct <= N and math.isfinite(res.loss_sum)
        eng.synchronize()
        out.append([eng.t[k].detach().cpu().clone() for k in ("params", "momentum", "loss_hist")])
    # (the last epoch's 25 steps ran; 200 images are soon fitted, a loss may round to 0)
    assert out[0][2][0] > 0 and torch.isfinite(out[0][2]).all() and out[0][1].abs().max() > 0
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.fixture(scope="module")
def trained():
    """16 SGD steps of batch 32 at lr 0.01 on the synthetic set (fp32 torch, CPU), 512 held-out
    images around the same prototypes, and the fp32 CPU model's logits on them."""
    from ddp_amd.data.mnist import synthetic_mnist, synthetic_mnist_test
    from ddp_amd.models import SimpleCNN

    torch.manual_seed(0)
    model = SimpleCNN()
    imgs, labels = synthetic_mnist(512)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    for s in range(16):
        x = imgs[32 * s:32 * s + 32].unsqueeze(1).float() / 255.0
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(x), labels[32 * s:32 * s + 32]).backward()
        opt.step()
    ti, tl = synthetic_mnist_test(512, n_train=512)
    with torch.no_grad():
        lg = model(ti.unsqueeze(1).float() / 255.0)
    return model, ti, tl, lg


@pytest.mark.parametrize("dtype,tol", [("bf16", 1e-2), ("fp32", 1e-3)])
def test_accuracy_against_the_fp32_cpu_model(C, trained, dtype, tol):
    from ddp_amd.data import DeviceMNIST
    from ddp_amd.engine import evaluate
    from ddp_amd.engine.evaluation import lowest_argmax
    from ddp_amd.models import SimpleCNN

    cpu_model, ti, tl, lg = trained
    top2 = lg.topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 2 * tol * lg.abs().max()).sum())
    want = int((lowest_argmax(lg) == tl).sum())
    gpu = SimpleCNN(compute_dtype=torch.float32 if dtype == "fp32" else torch.bfloat16).to(dev)
    gpu.load_state_dict(cpu_model.state_dict())
    res = evaluate(gpu, DeviceMNIST(ti, tl, dev), dev, dtype, batch_size=200)  # ragged: 200, 200, 112
    print(f"{dtype}: correct {res.correct} (oracle {want}) of 512, {near} images within the margin")
    assert near <= 0.25 * 512, "the oracle's margins are too small for this check to mean anything"
    assert res.count == 512 and abs(res.correct - want) <= near


def _two_rank_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from ddp_amd.data import DeviceMNIST
        from ddp_amd.data.mnist import synthetic_mnist_test
        from ddp_amd.engine import all_reduce_result, eval_shard, evaluate
        from ddp_amd.models import SimpleCNN

        torch.manual_seed(0)
        model = SimpleCNN().to(dev)
        imgs, labels = synthetic_mnist_test(101, n_train=101)
        data = DeviceMNIST(imgs, labels, dev)
        mine = evaluate(model, data, dev, "bf16", batch_size=16, indices=eval_shard(101, world, rank))
        tot = all_reduce_result(mine)
        own = [None] * world
        dist.all_gather_object(own, (int(mine.correct_rows.sum()), mine.count, tot.correct, tot.count, tot.loss_sum))
        assert tot.count == 101 and tot.correct == sum(o[0] for o in own) and sum(o[1] for o in own) == 101
        assert all(o[2:] == own[0][2:] for o in own)  # both ranks report the same totals
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, repr(e) + traceback.format_exc()[-600:]))


def test_two_ranks_on_one_gpu_exact_totals():
    from ddp_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res


def test_cli_eval_every_and_eval_only(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}

    def train(*args):
        cmd = [sys.executable, "-u", os.path.join(REPO, "train_ddp.py"), "--world_size", "1", "--data", "synthetic",
               "--device", "gpu", "--batch_size", "32", "--max_steps", "20", "--log_every", "1000", *args]
        p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=240)
        assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        return p.stdout

    out = train("--epochs", "2", "--eval_every", "1")
    lines = EVAL_LINE.findall(out)
    assert [m[0] for m in lines] == ["0", "1"], out
    assert all(m[4] == "10000" and 0 <= int(m[3]) <= 10000 for m in lines)
    out2 = train("--epochs", "2", "--eval_only")
    assert "Starting epoch" not in out2
    assert EVAL_LINE.findall(out2) == [lines[1]], out2
