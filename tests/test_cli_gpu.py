"""The default GPU CLI end to end on one MI355X (SURVEY §7.4 minimum
slice, BASELINE config 4 at world size 1): ``train_ddp.py`` on the fused native engine trains,
prints the reference's log lines (/root/reference/train_ddp.py:32-202, utils.py:14,19),
saves ``./checkpoints/epoch_N.pt`` in the reference schema (train_ddp.py:204-209),
auto-resumes on a re-run (train_ddp.py:45-185), and a crash + resume reproduces the
uninterrupted run's final checkpoint byte for byte (all zip records but the random
serialization_id), with and without momentum."""
import os
import subprocess
import sys
import zipfile

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train(cwd, *args, expect_rc=0, timeout=180):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, "-u", os.path.join(REPO, "train_ddp.py"), "--world_size", "1",
           "--data", "synthetic", "--device", "gpu", *args]
    p = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert p.returncode == expect_rc, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return p.stdout


def test_cli_train_save_resume(tmp_path):
    out = _train(tmp_path, "--epochs", "1", "--batch_size", "32", "--max_steps", "50",
                 "--log_every", "20")
    for line in ["Rank: 0 has initialized its process group with world size 1", "Rank 0 initialized",
                 "Rank 0 model wrapped in DDP", "Rank 0: Dataloader ready",
                 "Rank 0: Loss and Optimizer ready", "Rank 0: No checkpoint found, starting from scratch.",
                 "Rank 0: Starting epoch 0", "Epoch 0 | Batch 0 | Loss:", "Epoch 0 | Batch 40 | Loss:",
                 "Rank 0 cleaned up."]:
        assert line in out, (line, out)
    ck_dir = tmp_path / "checkpoints"
    assert sorted(os.listdir(ck_dir)) == ["epoch_0.pt"]
    ck = torch.load(ck_dir / "epoch_0.pt", weights_only=True)
    assert ck["epoch"] == 0 and list(ck) == ["epoch", "model", "optimizer"]
    for k, v in ck["model"].items():
        assert v.device.type == "cpu" and v.dtype == torch.float32 and torch.isfinite(v).all(), k
    # schema identical to the reference's own checkpoint (rebuilt from its recorded skeleton)
    from test_checkpoint import _reference_checkpoint

    (tmp_path / "reference").mkdir()
    ref_path = _reference_checkpoint(tmp_path / "reference", 0)
    ref = torch.load(ref_path, weights_only=True)
    assert list(ck["model"].keys()) == list(ref["model"].keys())
    assert ck["model"]._metadata == ref["model"]._metadata
    for k, v in ref["model"].items():
        assert ck["model"][k].shape == v.shape and ck["model"][k].stride() == v.stride(), k
    assert ck["optimizer"] == {"state": {}, "param_groups": ref["optimizer"]["param_groups"]}
    za, zb = zipfile.ZipFile(ref_path), zipfile.ZipFile(ck_dir / "epoch_0.pt")
    assert [i.filename for i in za.infolist()] == [i.filename for i in zb.infolist()]
    # re-run with more epochs: auto-resume at epoch 1
    out2 = _train(tmp_path, "--epochs", "2", "--batch_size", "32", "--max_steps", "30")
    assert "Rank 0: Starting epoch 1" in out2 and "Starting epoch 0" not in out2
    assert "No checkpoint found" not in out2
    assert sorted(os.listdir(ck_dir)) == ["epoch_0.pt", "epoch_1.pt"]
    ck1 = torch.load(ck_dir / "epoch_1.pt", weights_only=True)
    assert ck1["epoch"] == 1
    assert any(not torch.equal(ck1["model"][k], ck["model"][k]) for k in ck["model"])
    # nothing left to do: starts at epoch 2 >= epochs, no training, no new file
    out3 = _train(tmp_path, "--epochs", "2", "--batch_size", "32", "--max_steps", "30")
    assert "Starting epoch" not in out3 and sorted(os.listdir(ck_dir)) == ["epoch_0.pt", "epoch_1.pt"]


@pytest.mark.parametrize("momentum", ["0", "0.9"])
def test_cli_fault_resume_byte_identical(tmp_path, momentum):
    """Crash at epoch 1 step 20, re-run: epoch_2.pt == the uninterrupted run's.  The fused
    engine replays 16-step hipGraphs plus eager steps (--graph_steps 16, 40 steps/epoch)."""
    common = ["--epochs", "3", "--batch_size", "32", "--max_steps", "40", "--graph_steps", "16",
              "--momentum", momentum, "--log_every", "1000"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    _train(a, *common)
    out = _train(b, *common, "--fault_at", "1:20", expect_rc=17)
    assert "injected fault at epoch 1 step 20" in out
    assert sorted(os.listdir(b / "checkpoints")) == ["epoch_0.pt"]
    out = _train(b, *common)
    assert "Rank 0: Starting epoch 1" in out and "Starting epoch 0" not in out
    za = zipfile.ZipFile(a / "checkpoints" / "epoch_2.pt")
    zb = zipfile.ZipFile(b / "checkpoints" / "epoch_2.pt")
    diff = [i.filename for i in za.infolist() if za.read(i.filename) != zb.read(i.filename)]
    assert set(diff) <= {"epoch_2/.data/serialization_id"}, diff  # (the id may even coincide)
    ck = torch.load(a / "checkpoints" / "epoch_2.pt", weights_only=True)
    assert bool(ck["optimizer"]["state"]) == (momentum != "0")


@pytest.mark.parametrize("comm", ["xgmi", "rccl"])
def test_cli_fault_resume_dist_chain_byte_identical(tmp_path, comm):
    """VERDICT r4 missing #3 (BASELINE config 4 on the production multi-GPU chain): the
    default ws > 1 step chain (dist_mode 4) - the level-3 forward, the conv backward with the
    fc weight gradient as its third role and the fused slab reduction (reducers stop short of
    the SGD), then ONE launch all-reducing both buckets of the 8-rank plan side by side with
    the optimizer fused into its all-gather and carrying the next step's forward (xGMI: the
    step head) or RCCL + one SGD pass; plus the start-up chain check - rehearsed at world
    size 1 (--force_allreduce): a
    crash at epoch 1 step 20 and an auto-resume give the uninterrupted run's epoch_2.pt byte
    for byte, and that equals the one-GPU chain's.  (The same chain at 2 ranks on one GPU, on
    the level-1 forward that ranks sharing a device run:
    tests/test_cli_multirank_gpu.py::test_two_rank_fault_resume_byte_identical.)"""
    common = ["--epochs", "3", "--batch_size", "32", "--max_steps", "40", "--graph_steps", "16",
              "--momentum", "0.9", "--log_every", "1000"]
    dist = [*common, "--force_allreduce", "--comm", comm]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
    out = _train(a, *dist)
    assert "start-up chain check passed" in out, out
    out = _train(b, *dist, "--fault_at", "1:20", expect_rc=17)
    assert "injected fault at epoch 1 step 20" in out
    out = _train(b, *dist)
    assert "Rank 0: Starting epoch 1" in out and "Starting epoch 0" not in out
    _train(c, *common)  # the comm-free one-GPU chain
    for other in (b, c):
        za = zipfile.ZipFile(a / "checkpoints" / "epoch_2.pt")
        zb = zipfile.ZipFile(other / "checkpoints" / "epoch_2.pt")
        diff = [i.filename for i in za.infolist() if za.read(i.filename) != zb.read(i.filename)]
        assert set(diff) <= {"epoch_2/.data/serialization_id"}, (other, diff)


def test_torchrun_entrypoint_gpu(tmp_path):
    """VERDICT r3 missing #2: the reference's main entrypoint (README.md:52,69,77 - torchrun)
    on the GPU: torch.distributed.run with one worker runs train_ddp.py on the fused engine
    over RCCL (no nested spawn), prints the reference's log lines, saves, and a second
    torchrun launch auto-resumes at the next epoch."""
    from ddp_amd.parallel import free_port

    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}

    def torchrun(*args):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
               "--master-addr=127.0.0.1", f"--master-port={free_port()}",
               os.path.join(REPO, "train_ddp.py"), "--data", "synthetic", "--device", "gpu", *args]
        p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=240)
        assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        return p.stdout

    out = torchrun("--epochs", "1", "--max_steps", "30", "--log_every", "10")
    for line in ["Rank: 0 has initialized its process group with world size 1", "Rank 0 model wrapped in DDP",
                 "Rank 0: No checkpoint found, starting from scratch.", "Rank 0: Starting epoch 0",
                 "Epoch 0 | Batch 20 | Loss:", "Rank 0 cleaned up."]:
        assert line in out, (line, out)
    assert out.count("has initialized its process group") == 1  # no nested spawn under torchrun
    assert sorted(os.listdir(tmp_path / "checkpoints")) == ["epoch_0.pt"]
    out2 = torchrun("--epochs", "2", "--max_steps", "30")
    assert "Resumed from" in out2 and "Rank 0: Starting epoch 1" in out2 and "Starting epoch 0" not in out2
    assert sorted(os.listdir(tmp_path / "checkpoints")) == ["epoch_0.pt", "epoch_1.pt"]


def _bench(*args, timeout=240):
    import json

    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-u", os.path.join(REPO, "bench.py"), *args], cwd=REPO, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_fuse_level0_keeps_the_fp32_record():
    """``--fuse_level 0`` is an advertised choice; the exact-fp32 run after
    the bf16 headline has no level-0 chain and times level 1 instead of failing the bench."""
    r = _bench("--steps", "4", "--warmup", "1", "--fuse_level", "0", "--full")
    c = r["config"]
    assert r["n_gpus"] == 1 and r["value"] > 0 and c["fuse_level"] == 0
    assert c["fp32_images_per_sec"] and c["fp32_images_per_sec"] > 0


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run times the headline only (no exact-fp32 run: that is ``--full``'s), reports
    the step time of exactly ``--steps`` steps, and ``--dump-outputs`` writes the parameters
    after the last timed step and the loss history as float32 ``.npy`` files."""
    import numpy as np

    d = tmp_path / "out"
    r = _bench("--gpus", "1", "--steps", "6", "--warmup", "2", "--dump-outputs", str(d))
    c = r["config"]
    assert r["steps"] == 6 and r["ms_per_step"] > 0 and r["dtype"] == "bf16"
    assert abs(r["value"] - 32 * 1000.0 / r["ms_per_step"]) <= 1e-3 * r["value"]
    assert c["fp32_images_per_sec"] is None and c["step_breakdown"] is None
    assert sorted(os.listdir(d)) == ["loss_hist.npy", "params.npy"]
    p, h = np.load(d / "params.npy"), np.load(d / "loss_hist.npy")
    # (the flat parameter space: 520,586 parameters plus each tensor's alignment padding)
    assert p.dtype == np.float32 and p.ndim == 1 and 520586 <= p.size < 520586 + 6 * 64
    assert np.isfinite(p).all() and np.abs(p).max() > 0
    # 2 warm-up + 6 timed steps of one epoch window: 8 losses, the untouched rest is zero
    assert h.dtype == np.float32 and np.isfinite(h).all()
    assert (h[:8] > 0).all() and not h[8:].any()


def test_bench_forced_dist_record():
    """the multi-GPU chain timed on one GPU (``--force_allreduce``: world size
    1, the 8-rank bucket plan over the xGMI kernels) reports the one-stream chain the placement
    timing chose (both buckets' all-reduces in one launch, alone or carrying the next
    forward), the per-step
    breakdown against the comm-free engine, and the plan's cost source."""
    r = _bench("--steps", "20", "--warmup", "5", "--force_allreduce", "--no_fp32", "--full")
    c = r["config"]
    assert c["force_allreduce"] and c["bucket_allreduce"].startswith("xgmi")
    assert c["pair_allreduce"] and not c["inlaunch_allreduce"]
    # the placement timed on this GPU picks the chain: dist_mode 3 (3 kernels per step) or the
    # step head (4: 2 per step, plus the graph's first standalone forward)
    run = c["placement"]["dist_mode_run"]
    assert run in (3, 4), c["placement"]
    assert c["kernels_per_step"] == 3 if run == 3 else 2 < c["kernels_per_step"] < 2.2, c["kernels_per_step"]
    b = c["step_breakdown"]
    assert b["step_us"] > 0 and b["local_step_us"] > 0 and b["local_kernels_per_step"] == 2
    assert c["bucket_plan"]["cost_source"]
    assert c["params_finite"]
