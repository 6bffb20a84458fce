"""ResNet-18 held-out evaluation on MI355X: the fused conv + BatchNorm inference forward
(``ResNet.forward_infer``) through ``evaluate_resnet`` and the trainer's ``--eval_size``.

Whole network: no a-priori bound exists through 20 layers, so the yardstick is the EXISTING
eval-mode forward (``model.eval(); model(x)``: conv -> raw bf16 y -> bn_apply, two roundings
per layer) measured in the same test against the same float64 CPU logits; the fused path
rounds once per layer, so its max-abs logit error must not exceed 1.5 x the unfused path's
(the margin covers a different rounding pattern, not a worse one).  Both errors are printed
(run with -s) and recorded in profiles/resnet_eval/README.md.
"""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL5_LINE = re.compile(r"Epoch (\d+) \| Eval \| Loss: ([\d.]+|nan|inf) \| Accuracy: ([\d.]+)% \((\d+)/(\d+)\) "
                        r"\| Top-5: ([\d.]+)% \((\d+)/(\d+)\)")


def randomise_bn(model, seed=5):
    """Running statistics and affine parameters under which eval-mode BatchNorm is far from the
    identity: running_mean ~ N(0, 0.5), running_var in [0.5, 2], gamma in [0.5, 1.5], beta ~ N(0, 0.3)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.running_mean.copy_(torch.randn(C, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(C, generator=g) + 0.5)
                m.bias.copy_(torch.randn(C, generator=g) * 0.3)
    return model


@pytest.fixture(scope="module")
def net(C):
    """ResNet-18 for 64 x 64 images and 10 classes on the GPU, its float64 CPU twin holding the
    bf16-rounded conv weights, a batch of 3 images (bf16-rounded) and the twin's logits."""
    from ddp_amd.models import resnet18
    from ddp_amd.models.layers import Conv2d

    torch.manual_seed(0)
    model = randomise_bn(resnet18(num_classes=10)).to(dev)
    twin = resnet18(num_classes=10)
    twin.load_state_dict(model.state_dict())
    with torch.no_grad():
        for m in twin.modules():
            if isinstance(m, Conv2d):
                m.weight.copy_(m.weight.to(torch.bfloat16).float())
    twin = twin.double().eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(3, 3, 64, 64, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        ref = twin(x.double())
    return model, x.float().to(dev), ref


def test_whole_network_logits_fused_vs_unfused(net):
    from ddp_amd.ops.resnet_fn import to_nhwc4

    model, x, ref = net
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    fused = model.forward_infer(to_nhwc4(x))
    assert model.training and fused.dtype == torch.float32 and tuple(fused.shape) == (3, 10)
    model.eval()
    with torch.no_grad():
        unfused = model(x).float()
    model.train()
    torch.cuda.synchronize()
    ef = (fused.cpu().double() - ref).abs().max().item()
    eu = (unfused.cpu().double() - ref).abs().max().item()
    print(f"RESNET_EVAL logits max-abs error vs float64: fused {ef:.5f} unfused {eu:.5f} "
          f"(max |logit| {ref.abs().max().item():.3f})")
    assert eu > 0 and ref.abs().max().item() > 0.1
    assert ef <= 1.5 * eu, f"fused {ef} vs unfused {eu}"
    for k, v in model.state_dict().items():  # nothing was written
        assert torch.equal(v, state[k]), k


@pytest.fixture(scope="module")
def split(C):
    from ddp_amd.data import DeviceImages, synthetic_imagenet_test

    imgs, labels = synthetic_imagenet_test(37, 64, 10, seed=2, n_train=16)
    return DeviceImages(imgs, labels, dev)


def test_predictions_follow_the_rules(net, split):
    from ddp_amd.engine.evaluation import evaluate_resnet, lowest_argmax, top5_hit

    model = net[0]
    res = evaluate_resnet(model, split, batch_size=16, want_logits=True)
    lg, labels = res.logits, split.labels
    assert tuple(lg.shape) == (37, 10) and bool(torch.isfinite(lg).all())
    pred = lowest_argmax(lg).to(torch.int32)
    assert torch.equal(res.pred, pred)
    assert torch.equal(res.correct_rows, (pred == labels).to(torch.int32))
    assert torch.equal(res.correct5_rows, top5_hit(lg, labels))
    # the wave-per-row cross-entropy bound (tests/test_resnet_infer_gpu.py): (D + 64) u max(1, |ref|)
    x = lg.double()
    want = torch.logsumexp(x, 1) - x.gather(1, labels.view(-1, 1))[:, 0]
    D = (x - x.max(1, keepdim=True).values).abs().max(1).values
    assert bool(((res.loss.double() - want).abs() <= (D + 64) * 2.0 ** -24 * want.abs().clamp(min=1.0)).all())


def test_ragged_batches_counts_order_and_index_checks(net, split):
    from ddp_amd.engine.evaluation import evaluate_resnet

    model = net[0]
    res = evaluate_resnet(model, split, batch_size=16)  # 16 + 16 + 5
    assert res.count == 37 and res.logits is None
    assert res.correct == int(res.correct_rows.sum()) and res.correct5 == int(res.correct5_rows.sum())
    assert res.loss_sum == float(res.loss.double().cpu().cumsum(0)[-1])
    assert res.correct5 >= res.correct and res.top5 == res.correct5 / 37
    idx = torch.tensor([36, 0, 17, 17, 5, 20, 3])
    sub = evaluate_resnet(model, split, batch_size=3, indices=idx, want_logits=True)
    assert sub.count == 7
    for k in ("pred", "correct_rows", "correct5_rows"):
        assert torch.equal(getattr(sub, k), getattr(res, k)[idx.to(dev)]), k
    one = evaluate_resnet(model, split, batch_size=37, indices=idx, want_logits=True)
    assert torch.equal(one.pred, sub.pred)
    for bad in (torch.tensor([0, 37]), torch.tensor([-1]), torch.tensor([0.0, 1.0]), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            evaluate_resnet(model, split, batch_size=16, indices=bad)
    # the module engine (the unfused eval-mode forward) under the same rules
    mod = evaluate_resnet(model, split, batch_size=16, engine="module")
    assert mod.count == 37 and mod.correct5 is not None and model.training


def test_evaluation_leaves_no_trace_between_graphed_steps(split):
    """One graphed training step, an evaluation, another graphed step: parameters, momentum and
    BatchNorm buffers afterwards are bitwise those of the same two steps without the evaluation."""
    from ddp_amd.engine import GraphedStep
    from ddp_amd.engine.evaluation import evaluate_resnet
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(4, 3, 64, 64, generator=g).to(dev) for _ in range(2)]
    ys = [torch.randint(0, 10, (4,), generator=g).to(dev) for _ in range(2)]
    out = []
    for with_eval in (True, False):
        torch.manual_seed(0)
        model = resnet18(num_classes=10).to(dev)
        opt = FusedSGD(model, lr=0.05, momentum=0.9, weight_decay=1e-4)
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss

        gs = GraphedStep(step, (xs[0], ys[0]), warmup=1)
        gs(xs[1], ys[1])
        if with_eval:
            before = {k: v.clone() for k, v in model.state_dict().items()}
            grads = [p.grad.clone() if p.grad is not None else None for p in model.parameters()]
            res = evaluate_resnet(model, split, batch_size=16)
            assert res.count == 37 and model.training
            for k, v in model.state_dict().items():
                assert torch.equal(v, before[k]), k
            for p, g0 in zip(model.parameters(), grads):
                assert (p.grad is None) == (g0 is None) and (g0 is None or torch.equal(p.grad, g0))
        gs(xs[0], ys[0])
        gs(xs[1], ys[1])
        torch.cuda.synchronize()
        mom = getattr(opt, "momentum_buffer", None)
        out.append(([p.detach().clone() for p in model.parameters()], [b.clone() for b in model.buffers()],
                    mom.clone() if mom is not None else None))
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)
    assert out[0][2] is not None and torch.equal(out[0][2], out[1][2])


def test_cli_eval_size_eval_every_and_eval_only(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    metrics = str(tmp_path / "m.jsonl")

    def train(*args):
        cmd = [sys.executable, "-u", os.path.join(REPO, "train_ddp.py"), "--world_size", "1", "--device", "gpu",
               "--model", "resnet18", "--graph_module", "--image_size", "64", "--num_classes", "10",
               "--dataset_size", "64", "--batch_size", "16", "--log_every", "1000", "--epochs", "2",
               "--eval_size", "40", *args]
        p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=240)
        assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        return p.stdout

    out = train("--eval_every", "1", "--metrics_json", metrics)
    lines = EVAL5_LINE.findall(out)
    assert [m[0] for m in lines] == ["0", "1"], out
    assert "Rank 0: Eval split: synthetic (40 images)" in out
    for m in lines:
        assert m[4] == "40" == m[7] and 0 <= int(m[3]) <= int(m[6]) <= 40
    recs = [json.loads(ln) for ln in open(metrics)]
    assert len(recs) == 2
    for m, rec in zip(lines, recs):
        assert rec["eval_top5"] == int(m[6]) / 40 and rec["eval_accuracy"] == int(m[3]) / 40
    out2 = train("--eval_only")
    assert "Starting epoch" not in out2
    assert EVAL5_LINE.findall(out2) == [lines[1]], out2
