"""Held-out evaluation without a GPU: the test split (IDX files and the synthetic one), the
padding-free shard partition, and the CPU trainer's ``--eval_every`` - 2 gloo ranks whose
all-reduced counts equal a single-process evaluation of the saved checkpoints exactly."""
import gzip
import hashlib
import json
import os
import re
import struct

import pytest
import torch
import torch.multiprocessing as mp

from ddp_amd.data import load_mnist, synthetic_mnist
from ddp_amd.parallel import free_port

EVAL_LINE = re.compile(r"^Epoch (\d+) \| Eval \| Loss: (\d+\.\d{4}) \| Accuracy: (\d+\.\d{2})% \((\d+)/(\d+)\)$", re.M)


def _idx_bytes(t: torch.Tensor) -> bytes:
    return struct.pack(">HBB", 0, 0x08, t.dim()) + struct.pack(">" + "I" * t.dim(), *t.shape) + t.numpy().tobytes()


def _write_t10k(root, imgs, labels, gz):
    d = os.path.join(root, "MNIST", "raw")
    os.makedirs(d, exist_ok=True)
    for name, t in (("t10k-images-idx3-ubyte", imgs), ("t10k-labels-idx1-ubyte", labels)):
        op, path = (gzip.open, os.path.join(d, name + ".gz")) if gz else (open, os.path.join(d, name))
        with op(path, "wb") as f:
            f.write(_idx_bytes(t))


@pytest.mark.parametrize("gz", [False, True])
def test_load_mnist_test_split_reads_t10k_idx(tmp_path, gz):
    g = torch.Generator().manual_seed(3)
    imgs = torch.randint(0, 256, (7, 28, 28), generator=g).to(torch.uint8)
    labels = torch.randint(0, 10, (7,), generator=g).to(torch.uint8)
    _write_t10k(str(tmp_path), imgs, labels, gz)
    for source in ("mnist", "auto"):  # (auto: the test files exist, the train files do not)
        got_i, got_l, src = load_mnist(str(tmp_path), source, split="test")
        assert src == "mnist" and got_i.dtype == torch.uint8 and got_l.dtype == torch.int64
        assert torch.equal(got_i, imgs) and torch.equal(got_l, labels.long())
    # the train side decides for itself: no train files here -> synthetic under auto, an error under mnist
    assert load_mnist(str(tmp_path), "auto")[2] == "synthetic"
    with pytest.raises(FileNotFoundError):
        load_mnist(str(tmp_path), "mnist")
    with pytest.raises(ValueError):
        load_mnist(str(tmp_path), "auto", split="validation")


def test_load_mnist_test_split_wrong_shapes_raise(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    _write_t10k(str(a), torch.zeros(4, 14, 14, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8), False)
    with pytest.raises(ValueError):
        load_mnist(str(a), "mnist", split="test")
    _write_t10k(str(b), torch.zeros(4, 28, 28, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8), False)
    with pytest.raises(ValueError):
        load_mnist(str(b), "mnist", split="test")


def test_synthetic_train_split_unchanged(tmp_path):
    """The train generator's output is what it was before the test split existed (a digest
    recorded from the parent commit), and load_mnist's default split still returns it."""
    i, l = synthetic_mnist(2048)
    digest = hashlib.sha256(i.numpy().tobytes() + l.numpy().tobytes()).hexdigest()
    assert digest == "582632c257d890e5461420fc7760e8be5b8d7f3e484599c85f49d2d640e84db1"
    ref_i, ref_l = synthetic_mnist()
    for kw in ({}, {"split": "train"}):
        got_i, got_l, src = load_mnist(str(tmp_path), "synthetic", **kw)
        assert src == "synthetic" and torch.equal(got_i, ref_i) and torch.equal(got_l, ref_l)


def test_synthetic_test_split():
    ti, tl, src = load_mnist("/nonexistent", "auto", split="test")
    ti2, tl2, _ = load_mnist("/nonexistent", "synthetic", split="test")
    assert src == "synthetic" and torch.equal(ti, ti2) and torch.equal(tl, tl2)  # deterministic
    assert ti.shape == (10000, 28, 28) and ti.dtype == torch.uint8 and tl.shape == (10000,)
    assert sorted(tl.unique().tolist()) == list(range(10))
    tri, trl = synthetic_mnist()
    assert not torch.equal(ti, tri[:10000])  # its own labels and noise
    # same class prototypes: a 1,000-image class mean carries ~0.8 grey levels of noise,
    # different prototypes differ by tens
    for c in range(10):
        a = ti[tl == c].float().mean(0)
        b = tri[trl == c].float().mean(0)
        assert (a - b).abs().max().item() <= 8.0, c
        other = tri[trl == (c + 1) % 10].float().mean(0)
        assert (a - other).abs().max().item() > 8.0, c


@pytest.mark.parametrize("n", [10, 10000])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_eval_shard_is_an_exact_partition(n, world):
    from ddp_amd.engine import eval_shard

    shards = [eval_shard(n, world, r) for r in range(world)]
    assert torch.equal(torch.cat(shards).sort().values, torch.arange(n))  # every sample exactly once
    sizes = [s.numel() for s in shards]
    assert max(sizes) - min(sizes) <= 1 and sum(sizes) == n
    with pytest.raises(ValueError):
        eval_shard(n, world, world)


def test_lowest_argmax_and_forward_path_tie_rule():
    from ddp_amd.data import DeviceMNIST
    from ddp_amd.engine import EvalResult, evaluate
    from ddp_amd.engine.evaluation import lowest_argmax
    from ddp_amd.models import SimpleCNN

    lg = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 2.0, 2.0]])
    assert lowest_argmax(lg).tolist() == [1, 0, 2]
    model = SimpleCNN()
    with torch.no_grad():
        model.fl.weight.zero_()
        model.fl.bias.zero_()
    imgs, labels = synthetic_mnist(37)
    res = evaluate(model, DeviceMNIST(imgs, labels, "cpu"), batch_size=16)  # ragged: 16, 16, 5
    assert isinstance(res, EvalResult) and res.count == 37
    assert res.pred.tolist() == [0] * 37 and res.correct == int((labels == 0).sum())
    assert abs(res.loss_sum - 37 * torch.log(torch.tensor(10.0)).item()) < 1e-4
    assert model.training  # (the mode is restored)


def _worker_eval_train(rank, ws, port, ckdir, metrics, eval_every):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import TrainOptions, ddp_train

    opts = TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, max_steps=3, num_workers=0,
                        log_every=1000, data="synthetic", metrics_json=metrics, eval_every=eval_every,
                        eval_batch_size=1000)
    ddp_train(rank, ws, 2, 32, opts)


@pytest.mark.slow
def test_cpu_trainer_eval_every_counts_are_exact(tmp_path, capfd):
    from ddp_amd.data import DeviceMNIST
    from ddp_amd.engine import eval_shard, evaluate
    from ddp_amd.models import SimpleCNN

    ck, metrics = str(tmp_path / "ck"), str(tmp_path / "m.jsonl")
    mp.start_processes(_worker_eval_train, args=(2, free_port(), ck, metrics, 1), nprocs=2,
                       start_method="spawn", join=True)
    out = capfd.readouterr().out
    lines = EVAL_LINE.findall(out)
    assert [int(m[0]) for m in lines] == [0, 1], out  # one line per epoch, rank 0 only
    assert "Rank 0: Eval split: synthetic (10000 images)" in out
    recs = [json.loads(ln) for ln in open(metrics)]
    assert len(recs) == 2
    ti, tl, _ = load_mnist("/nonexistent", "synthetic", split="test")
    data = DeviceMNIST(ti, tl, "cpu")
    for (epoch, loss, acc, correct, count), rec in zip(lines, recs):
        model = SimpleCNN()
        model.load_state_dict(torch.load(os.path.join(ck, f"epoch_{epoch}.pt"), weights_only=True)["model"])
        # the same fp32 torch forward per image on both sides: the ranks' shards, the ranks' batches
        parts = [evaluate(model, data, batch_size=1000, indices=eval_shard(10000, 2, r)) for r in range(2)]
        assert int(count) == 10000 == sum(p.count for p in parts)
        assert int(correct) == sum(p.correct for p in parts)
        assert abs(float(loss) - sum(p.loss_sum for p in parts) / 10000) < 1e-4
        assert float(acc) == round(100.0 * int(correct) / 10000, 2)
        assert rec["eval_accuracy"] == int(correct) / 10000 and abs(rec["eval_loss"] - float(loss)) < 1e-4


@pytest.mark.slow
def test_cpu_trainer_without_the_flag_is_unchanged(tmp_path, capfd):
    ck, metrics = str(tmp_path / "ck"), str(tmp_path / "m.jsonl")
    mp.start_processes(_worker_eval_train, args=(2, free_port(), ck, metrics, 0), nprocs=2,
                       start_method="spawn", join=True)
    out = capfd.readouterr().out
    assert "Eval" not in out
    recs = [json.loads(ln) for ln in open(metrics)]
    assert len(recs) == 2
    for rec in recs:
        assert sorted(rec) == ["batch_size", "epoch", "images_per_sec_aggregate", "samples_per_rank", "seconds",
                               "steps", "world_size"]


def test_resnet18_eval_every_raises(tmp_path):
    import train_ddp
    from ddp_amd.engine.trainer import TrainOptions, ddp_train

    with pytest.raises(ValueError, match="resnet18"):
        train_ddp.main(["--model", "resnet18", "--eval_every", "1", "--world_size", "1", "--device", "cpu",
                        "--checkpoint_dir", str(tmp_path)])
    with pytest.raises(ValueError, match="resnet18"):
        ddp_train(0, 1, 1, 8, TrainOptions(model="resnet18", eval_only=True, checkpoint_dir=str(tmp_path)))


def test_infer_tu_is_scratch_and_spill_free():
    """The inference TU like every other kernel TU (tests/test_kernel_resources_cpu.py): all
    four simplecnn_infer instantiations (bf16 / fp32 x pxt 1 / 2) and the totals kernel, no
    private segment, no VGPR spill."""
    from ddp_amd import _build
    from ddp_amd.utils import kernel_resources as kr

    _build.build(verbose=False)  # incremental: a no-op when the tree is built
    obj = os.path.join(_build.BUILD_DIR, "k_infer.hip.o")
    ks = kr.parse_kernels(kr.code_object_notes(obj))
    names = [k["name"] for k in ks]
    assert sum("simplecnn_infer_kernel" in n for n in names) == 4 and any("infer_totals_kernel" in n for n in names)
    bad = kr.offenders({"infer.hip": ks})
    assert not bad, [(n, k.get("private_segment_fixed_size"), k.get("vgpr_spill_count")) for _, n, k in bad]
