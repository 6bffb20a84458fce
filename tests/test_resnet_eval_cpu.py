"""ResNet-18 held-out evaluation without a GPU: the synthetic held-out split, the CPU
(module-forward) evaluator's top-1 / top-5 against an independent computation, the
``--eval_size`` flag's validation, the CPU trainer's Eval line and a 2-rank gloo run whose
totals are exact."""
import json
import os
import re

import pytest
import torch
import torch.multiprocessing as mp

from ddp_amd.parallel import free_port

EVAL5_LINE = re.compile(r"Epoch (\d+) \| Eval \| Loss: ([\d.]+|nan|inf) \| Accuracy: ([\d.]+)% \((\d+)/(\d+)\) "
                        r"\| Top-5: ([\d.]+)% \((\d+)/(\d+)\)")


def test_synthetic_imagenet_test_split():
    from ddp_amd.data import synthetic_imagenet, synthetic_imagenet_test

    ti, tl = synthetic_imagenet_test(24, 16, 7, seed=3, n_train=40)
    ti2, tl2 = synthetic_imagenet_test(24, 16, 7, seed=3, n_train=40)
    assert torch.equal(ti, ti2) and torch.equal(tl, tl2)  # deterministic
    assert ti.dtype == torch.uint8 and tuple(ti.shape) == (24, 16, 16, 3) and tl.dtype == torch.int64
    assert int(tl.min()) >= 0 and int(tl.max()) < 7
    # the train split's class colours: the noise is uniform in [-32, 32] around a colour in
    # [32, 223] (nothing clamps), so the pixels of one class span at most 64 per channel - over
    # BOTH splits together only if the test split draws around the same colours
    tri, trl = synthetic_imagenet(40, 16, 7, seed=3)
    shared = 0
    for c in range(7):
        a, b = tri[trl == c].reshape(-1, 3).int(), ti[tl == c].reshape(-1, 3).int()
        if not (a.numel() and b.numel()):
            continue
        shared += 1
        both = torch.cat([a, b])
        assert int((both.max(0).values - both.min(0).values).max()) <= 64, c
        assert int((b.max(0).values - b.min(0).values).min()) >= 48, "the test images carry the noise"
    assert shared >= 5
    # no test image equals a train image; another seed gives another split
    flat_train = {bytes(t.numpy().tobytes()) for t in tri}
    assert all(bytes(t.numpy().tobytes()) not in flat_train for t in ti)
    assert not torch.equal(synthetic_imagenet_test(24, 16, 7, seed=4, n_train=40)[0], ti)


def _tiny(seed=0):
    from ddp_amd.models import resnet18

    torch.manual_seed(seed)
    return resnet18(num_classes=7)


def test_cpu_evaluate_resnet_matches_an_independent_computation():
    from ddp_amd.data import DeviceImages, synthetic_imagenet_test
    from ddp_amd.engine.evaluation import _check_activation_sizes, evaluate_resnet

    model = _tiny()
    imgs, labels = synthetic_imagenet_test(11, 32, 7, seed=1, n_train=16)
    data = DeviceImages(imgs, labels, "cpu")
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    res = evaluate_resnet(model, data, batch_size=4, want_logits=True)  # 4 + 4 + 3
    assert model.training and res.count == 11
    for k, v in model.state_dict().items():  # eval-mode BatchNorm: no statistic moved
        assert torch.equal(v, state[k]), k
    model.eval()
    with torch.no_grad():
        lg = model(imgs.permute(0, 3, 1, 2).float() / 255.0)
    model.train()
    assert torch.allclose(res.logits, lg, atol=1e-5)
    # independent: torch.topk on rows without ties among the first five places
    top = res.logits.topk(6, dim=1).values
    assert bool((top[:, :-1] > top[:, 1:]).all()), "a tie in this seed's logits: pick another seed"
    top5 = res.logits.topk(5, dim=1).indices
    assert res.correct == int((res.logits.argmax(1) == labels).sum())
    assert res.correct5 == int((top5 == labels.view(-1, 1)).any(1).sum())
    assert torch.equal(res.correct5_rows, (top5 == labels.view(-1, 1)).any(1).to(torch.int32))
    assert res.top5 == res.correct5 / 11 and res.correct5 >= res.correct
    want = torch.nn.functional.cross_entropy(res.logits.double(), labels, reduction="sum").item()
    assert abs(res.loss_sum - want) < 1e-4
    idx = torch.tensor([10, 2, 2])
    sub = evaluate_resnet(model, data, batch_size=2, indices=idx)
    assert torch.equal(sub.pred, res.pred[idx]) and sub.count == 3
    with pytest.raises(ValueError):
        evaluate_resnet(model, data, indices=torch.tensor([11]))
    with pytest.raises(ValueError):
        evaluate_resnet(model, data, engine="nope")
    # the kernels index pixels with int: a batch with an activation of 2^31 elements is refused
    _check_activation_sizes(model, 1000, (224, 224))
    with pytest.raises(ValueError, match="2\\^31"):
        _check_activation_sizes(model, 2700, (224, 224))  # stem output: 2700 * 112 * 112 * 64 > 2^31


def test_top5_rule_with_ties_and_few_classes():
    from ddp_amd.engine.evaluation import EvalResult, top5_hit

    lg = torch.tensor([[9., 8., 7., 6., 5., 5., 0.], [9., 8., 7., 6., 5., 5., 0.], [1., 1., 1., 1., 1., 1., 1.]])
    assert top5_hit(lg, torch.tensor([4, 5, 5])).tolist() == [1, 0, 0]
    assert top5_hit(lg[:, :4], torch.tensor([3, 0, 3])).tolist() == [1, 1, 1]
    r = EvalResult(1, 2, 0.5)  # every earlier construction stays valid
    assert r.correct5 is None and r.correct5_rows is None and r.top5 != r.top5


def test_eval_size_validation(tmp_path):
    import train_ddp
    from ddp_amd.engine.trainer import TrainOptions, validate_options

    with pytest.raises(ValueError, match="eval_size"):
        train_ddp.main(["--model", "simplecnn", "--eval_size", "8", "--eval_every", "1", "--world_size", "1",
                        "--device", "cpu", "--checkpoint_dir", str(tmp_path)])
    with pytest.raises(ValueError, match="eval_size"):
        validate_options(TrainOptions(eval_size=8))
    with pytest.raises(ValueError, match="resnet18"):
        validate_options(TrainOptions(model="resnet18", eval_every=1))
    validate_options(TrainOptions(model="resnet18", eval_every=1, eval_size=8))


def _worker(rank, ws, port, ckdir, metrics, eval_size):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import TrainOptions, ddp_train

    opts = TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, max_steps=1, log_every=1000,
                        model="resnet18", image_size=32, num_classes=7, dataset_size=8, metrics_json=metrics,
                        eval_every=1, eval_size=eval_size, eval_batch_size=4)
    ddp_train(rank, ws, 1, 4, opts)


@pytest.mark.slow
def test_cpu_trainer_prints_the_eval_line(tmp_path, capfd):
    ck, metrics = str(tmp_path / "ck"), str(tmp_path / "m.jsonl")
    mp.start_processes(_worker, args=(1, free_port(), ck, metrics, 8), nprocs=1, start_method="spawn", join=True)
    out = capfd.readouterr().out
    lines = EVAL5_LINE.findall(out)
    assert len(lines) == 1 and lines[0][0] == "0" and lines[0][4] == "8" == lines[0][7], out
    assert "Rank 0: Eval split: synthetic (8 images)" in out
    rec = json.loads(open(metrics).read().strip())
    assert rec["eval_top5"] == int(lines[0][6]) / 8 and rec["eval_accuracy"] == int(lines[0][3]) / 8


@pytest.mark.slow
def test_two_gloo_ranks_report_exact_totals(tmp_path, capfd):
    from ddp_amd.data import DeviceImages, synthetic_imagenet_test
    from ddp_amd.engine import eval_shard
    from ddp_amd.engine.evaluation import evaluate_resnet
    from ddp_amd.models import resnet18

    ck, metrics = str(tmp_path / "ck"), str(tmp_path / "m.jsonl")
    N = 9  # odd: the shards differ in size
    mp.start_processes(_worker, args=(2, free_port(), ck, metrics, N), nprocs=2, start_method="spawn", join=True)
    out = capfd.readouterr().out
    lines = EVAL5_LINE.findall(out)
    assert len(lines) == 1, out  # rank 0 only
    _, loss, _, correct, count, _, correct5, count5 = lines[0]
    assert int(count) == N == int(count5)
    model = resnet18(num_classes=7)
    model.load_state_dict(torch.load(os.path.join(ck, "epoch_0.pt"), weights_only=True)["model"])
    imgs, labels = synthetic_imagenet_test(N, 32, 7, n_train=8)
    data = DeviceImages(imgs, labels, "cpu")
    parts = [evaluate_resnet(model, data, batch_size=4, indices=eval_shard(N, 2, r)) for r in range(2)]
    assert sum(p.count for p in parts) == N
    assert int(correct) == sum(int(p.correct_rows.sum()) for p in parts)
    assert int(correct5) == sum(int(p.correct5_rows.sum()) for p in parts)
    assert abs(float(loss) - sum(p.loss_sum for p in parts) / N) < 1e-4
