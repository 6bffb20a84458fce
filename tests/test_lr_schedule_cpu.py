"""Learning-rate schedules (--lr_schedule / --warmup_steps) without a GPU: the closed forms of
ddp_amd.ops.lr_schedule against torch.optim.lr_scheduler, FusedSGD(lr_schedule=) on the CPU
against torch.optim.SGD driven by the torch scheduler, the optimizer state, crash and resume over
two gloo ranks, and the fused engine's refusal.  Nothing here is calibrated on the code under test."""
import json
import os

import pytest
import torch
import torch.multiprocessing as mp
from torch.optim import lr_scheduler as tls

from ddp_amd.models import SimpleCNN
from ddp_amd.ops import kernel_bounds as kb
from ddp_amd.ops.lr_schedule import LRSchedule
from ddp_amd.parallel import free_port

U = kb.U
BASE, LR_MIN, WSTART = 0.1, 1e-4, 0.01


def torch_rates(kind, total, warmup, base=BASE, lr_min=LR_MIN, step_size=0, gamma=0.1, dtype=torch.float64):
    """The per-step rates torch.optim.lr_scheduler produces: ``kind`` after a SequentialLR
    LinearLR warm-up, stepped once per optimizer step; entry t is the rate step t runs at."""
    w = torch.nn.Parameter(torch.zeros(1, dtype=dtype))
    opt = torch.optim.SGD([w], lr=base)
    T = max(1, total - warmup)
    if kind == "cosine":
        main = tls.CosineAnnealingLR(opt, T_max=T, eta_min=lr_min)
    elif kind == "linear":
        main = tls.LinearLR(opt, start_factor=1.0, end_factor=lr_min / base, total_iters=T)
    elif kind == "step":
        main = tls.StepLR(opt, step_size=step_size, gamma=gamma)
    else:
        main = tls.ConstantLR(opt, factor=1.0, total_iters=0)
    sched = main
    if warmup:
        warm = tls.LinearLR(opt, start_factor=WSTART, end_factor=1.0, total_iters=warmup)
        sched = tls.SequentialLR(opt, [warm, main], milestones=[warmup])
    rates = []
    for _ in range(total):
        rates.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return rates


# ------------------------------------------------------------------ closed forms against torch
@pytest.mark.parametrize("total,warmup", [(500, 0), (500, 37), (4000, 100)])
@pytest.mark.parametrize("kind", ["cosine", "step", "linear"])
def test_closed_forms_match_torch_schedulers(kind, total, warmup):
    """Relative error <= 1e-11 in float64 (torch's schedulers are recursive - each step rescales
    the previous rate - so they carry a few ulps per step: ~1e-13 over these lengths), and not
    one float32 table entry differs from the rounding of torch's value."""
    import warnings

    step_size = 120
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # SequentialLR's own deprecation notice about step(epoch)
        ref = torch.tensor(torch_rates(kind, total, warmup, step_size=step_size), dtype=torch.float64)
    s = LRSchedule(BASE, total, kind, warmup_steps=warmup, warmup_start=WSTART, lr_min=LR_MIN,
                   step_size=step_size, gamma=0.1)
    assert s.values.dtype == torch.float64 and s.table.dtype == torch.float32 and len(s) == total
    rel = ((s.values - ref).abs() / ref.abs()).max().item()
    mism = int((s.table != ref.to(torch.float32)).sum())
    print(f"LR_SCHED {kind} total={total} warmup={warmup} max_rel={rel:.3e} fp32_mismatch={mism}")
    assert rel <= 1e-11, rel
    assert mism == 0
    assert torch.equal(s.table, s.values.to(torch.float32))
    if warmup:
        assert s.values[0].item() == pytest.approx(BASE * WSTART, rel=1e-15)
        assert s.values[warmup].item() == BASE  # k = 0 of every decay is the base rate
    if kind == "cosine":  # ends one step short of lr_min, as CosineAnnealingLR at T_max - 1
        assert LR_MIN < s.values[-1].item() < s.values[-2].item() < BASE


def test_none_kind_is_constant_after_warmup_and_from_values_and_the_end_holds():
    s = LRSchedule(0.05, 10, "none", warmup_steps=4)
    assert s.values[4:].tolist() == [0.05] * 6 and s.values[:4].tolist() == sorted(s.values[:4].tolist())
    assert s.values[0].item() == pytest.approx(0.05 * 0.01)
    v = LRSchedule.from_values([0.3, 0.2, 0.1])
    assert len(v) == 3 and v.table.tolist() == torch.tensor([0.3, 0.2, 0.1]).tolist()
    assert [v.lr_at(t) for t in (0, 2, 3, 10 ** 9)] == [v.table[0].item(), v.table[2].item()] + [v.table[2].item()] * 2
    for bad in (dict(kind="exp"), dict(total_steps=0), dict(kind="step"), dict(warmup_steps=-1)):
        kw = dict(base_lr=0.1, total_steps=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            LRSchedule(**kw)
    with pytest.raises(ValueError):
        LRSchedule.from_values([])


# ------------------------------------------------------------------------ FusedSGD on CPU
def _batches(k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(8, 1, 28, 28, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(k)]


@pytest.mark.parametrize("kind,warmup", [("cosine", 3), ("step", 0), ("linear", 2)])
def test_fused_sgd_cpu_follows_the_torch_scheduler(kind, warmup):
    """FusedSGD(lr_schedule=) with momentum 0.9 and weight decay, 12 steps over an 8-step
    schedule, against torch.optim.SGD in float64 whose lr is set each step by the matching torch
    scheduler (held at its last value once the schedule has ended), fed the SAME fp32 gradients -
    the pattern and the tolerance of test_grad_clip_cpu.py's FusedSGD test: the per-step rounding
    bounds of kernel_bounds.sgd_bounds carried through the steps,

        gradient      E_d    = wd E_p                    (d = g + wd p; g is shared)
        momentum      E_buf' = m E_buf + E_d + 4 u BUF   (kernel_bounds.sgd_bounds)
        parameter     E_p'   = E_p + lr E_buf' + 6 u P

    The rate's own rounding (the table is fp32: relative error u) is one of the roundings that
    6 u P counts: p' = fl(p - fl(lr) d)."""
    from ddp_amd.ops import FusedSGD

    total, steps, mom, wd, base = 8, 12, 0.9, 5e-3, 0.1
    ref_rates = torch_rates(kind, total, warmup, base=base, lr_min=1e-3, step_size=3, gamma=0.5)
    sched = LRSchedule(base, total, kind, warmup_steps=warmup, lr_min=1e-3, step_size=3, gamma=0.5)
    torch.manual_seed(3)
    model = SimpleCNN()
    opt = FusedSGD(model, lr=base, momentum=mom, weight_decay=wd, lr_schedule=sched)
    fs = opt.flat
    ref = [torch.nn.Parameter(fs.view(fs.params, n).detach().double().clone()) for n in fs.names]
    topt = torch.optim.SGD(ref, lr=base, momentum=mom, weight_decay=wd)
    E_p = torch.zeros(fs.numel, dtype=torch.float64)
    E_buf = torch.zeros(fs.numel, dtype=torch.float64)
    used = []
    for k, (x, y) in enumerate(_batches(steps)):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        fs.reattach_grads()
        for n, r in zip(fs.names, ref):
            r.grad = fs.view(fs.grads, n).detach().double().clone()
        g64, p64 = fs.grads.double().clone(), fs.params.double().clone()
        m_prev = opt.momentum_buffer.double().clone() if opt.momentum_buffer is not None else torch.zeros_like(g64)
        lr = ref_rates[min(k, total - 1)]
        topt.param_groups[0]["lr"] = lr
        assert opt.schedule_step() == k
        assert opt.current_lr() == sched.table[min(k, total - 1)].item()
        assert abs(opt.current_lr() - lr) <= U * lr  # the table's one fp32 rounding of torch's rate
        used.append(opt.current_lr())
        topt.step()
        opt.step()
        bp, bb = kb.sgd_bounds(p64, g64, m_prev, lr, mom, 0.0, wd, False, k == 0)
        E_buf = (mom * E_buf if k else 0) + wd * E_p + bb
        E_p = E_p + lr * E_buf + bp
        for n, r in zip(fs.names, ref):
            err = (fs.view(fs.params, n).detach().double() - r.detach()).abs()
            bound = fs.view(E_p, n)
            assert bool((err <= bound).all()), (k, n, (err / (bound + 1e-300)).max().item())
    assert opt.schedule_step() == steps
    assert used[total - 1:] == [sched.table[-1].item()] * (steps - total + 1), "the last rate holds past the end"
    assert len(set(used[:total])) > 2  # (and the rate did move)
    # a schedule is not optional plumbing: the same run at the constant base rate ends elsewhere
    torch.manual_seed(3)
    m2 = SimpleCNN()
    o2 = FusedSGD(m2, lr=base, momentum=mom, weight_decay=wd)
    for x, y in _batches(steps):
        o2.zero_grad()
        torch.nn.functional.cross_entropy(m2(x), y).backward()
        o2.step()
    assert not torch.equal(o2.flat.params, fs.params)


# ------------------------------------------------------------------------ optimizer state
def _run(schedule, steps=3, lr=0.1):
    from ddp_amd.ops import FusedSGD

    torch.manual_seed(5)
    m = SimpleCNN()
    o = FusedSGD(m, lr=lr, momentum=0.9, lr_schedule=schedule)
    for x, y in _batches(steps):
        o.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        o.step()
    return m, o


def test_state_dict_keeps_its_keys_and_carries_the_next_rate():
    from ddp_amd.ops import FusedSGD

    sched = LRSchedule(0.1, 10, "cosine", warmup_steps=2)
    _, plain = _run(None)
    _, so = _run(sched)
    a, b = plain.state_dict(), so.state_dict()
    assert list(a) == list(b) and sorted(a["state"]) == sorted(b["state"])
    assert list(a["param_groups"][0]) == list(b["param_groups"][0])
    for i in a["state"]:
        assert list(a["state"][i]) == list(b["state"][i]) == ["momentum_buffer"]
    assert so.schedule_step() == 3
    assert b["param_groups"][0]["lr"] == sched.table[3].item() == so.current_lr()
    assert a["param_groups"][0]["lr"] == 0.1 == plain.current_lr()
    # set_schedule_step round-trips, and the state dict follows it
    for k in (0, 7, 9, 10, 55):
        so.set_schedule_step(k)
        assert so.schedule_step() == k
        assert so.state_dict()["param_groups"][0]["lr"] == sched.table[min(k, 9)].item()
    with pytest.raises(ValueError):
        so.set_schedule_step(-1)
    with pytest.raises(RuntimeError):
        plain.set_schedule_step(1)
    with pytest.raises(RuntimeError):
        plain.schedule_step()
    # load: the base rate is the constructor's, never a checkpoint's point of the schedule
    so.set_schedule_step(3)
    fresh = FusedSGD(SimpleCNN(), lr=0.1, momentum=0.9, lr_schedule=LRSchedule(0.1, 10, "cosine", warmup_steps=2))
    fresh.load_state_dict(so.state_dict())
    assert fresh.param_groups[0]["lr"] == 0.1 and fresh.schedule_step() == 0
    assert fresh.loaded_lr == sched.table[3].item()  # kept, so a resume can check its step index against it
    assert torch.equal(fresh.momentum_buffer, so.momentum_buffer)
    fresh.set_schedule_step(3)
    assert fresh.state_dict()["param_groups"] == so.state_dict()["param_groups"]
    # without a schedule a checkpoint's lr is taken, as before
    off = FusedSGD(SimpleCNN(), lr=0.5, momentum=0.9)
    off.load_state_dict(so.state_dict())
    assert off.param_groups[0]["lr"] == sched.table[3].item()


# ------------------------------------------------------------------------ crash and resume
def _worker_fault(rank, ws, port, ckdir, epochs, fault, metrics=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import TrainOptions, ddp_train

    opts = TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, max_steps=12, num_workers=0,
                        log_every=1000, data="synthetic", fault=fault, momentum=0.9, lr=0.05,
                        lr_schedule="cosine", warmup_steps=3, lr_min=1e-4, metrics_json=metrics)
    ddp_train(rank, ws, epochs, 32, opts)


@pytest.mark.slow
def test_fault_then_resume_is_byte_identical_with_a_schedule(tmp_path, capfd):
    """test_ddp_cpu.py::test_fault_then_resume_is_byte_identical with --lr_schedule cosine
    --warmup_steps 3: a crash in epoch 1, auto-resume (which restores the schedule's step index
    from the epoch alone), and the final checkpoint equals the uninterrupted run's - every zip
    record except the random serialization_id.  The uninterrupted run's per-epoch ``lr`` records
    are the table's entries at the epoch boundaries."""
    import zipfile

    a, b, metrics = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "m.jsonl")
    mp.start_processes(_worker_fault, args=(2, free_port(), a, 3, None, metrics), nprocs=2,
                       start_method="spawn", join=True)
    with pytest.raises(Exception):
        mp.start_processes(_worker_fault, args=(2, free_port(), b, 3, (1, 5, 1)), nprocs=2,
                           start_method="spawn", join=True)
    assert sorted(os.listdir(b)) == ["epoch_0.pt"]
    mp.start_processes(_worker_fault, args=(2, free_port(), b, 3, None), nprocs=2,
                       start_method="spawn", join=True)
    out = capfd.readouterr().out
    assert "Resumed from" in out and "WARNING" not in out  # the checkpoint's lr is the table's rate at the restored step
    za, zb = zipfile.ZipFile(os.path.join(a, "epoch_2.pt")), zipfile.ZipFile(os.path.join(b, "epoch_2.pt"))
    diff = [i.filename for i in za.infolist() if za.read(i.filename) != zb.read(i.filename)]
    assert set(diff) <= {"epoch_2/.data/serialization_id"}, diff
    table = LRSchedule(0.05, 36, "cosine", warmup_steps=3, lr_min=1e-4).table
    recs = [json.loads(ln) for ln in open(metrics)]
    assert [r["lr"] for r in recs] == [table[12].item(), table[24].item(), table[35].item()]
    for e in range(3):
        ck = torch.load(os.path.join(a, f"epoch_{e}.pt"), weights_only=True)
        assert ck["optimizer"]["param_groups"][0]["lr"] == recs[e]["lr"]
    assert len({r["lr"] for r in recs}) == 3


# ------------------------------------------------------------------------------------ CLI
def test_cli_fused_engine_refuses_schedules_and_the_default_builds_none():
    import train_ddp
    from ddp_amd.engine.trainer import (TrainOptions, build_lr_schedule, check_fused_engine_options,
                                        optimizer_steps_per_epoch, uses_lr_schedule, validate_options)

    d = train_ddp.parse_args([])
    assert (d.lr_schedule, d.warmup_steps, d.lr_min, d.lr_step_epochs, d.lr_gamma) == ("none", 0, 0.0, 0, 0.1)
    for flags in (["--lr_schedule", "cosine"], ["--warmup_steps", "2"]):
        with pytest.raises(ValueError, match="--engine module"):
            train_ddp.main(flags + ["--engine", "fused", "--device", "gpu"])
    for kw in (dict(lr_schedule="cosine"), dict(warmup_steps=2)):
        with pytest.raises(ValueError, match="--engine module"):  # what every rank checks once it knows its device
            check_fused_engine_options(TrainOptions(engine="fused", **kw), fused=True)
        check_fused_engine_options(TrainOptions(engine="fused", **kw), fused=False)  # the CPU path
        validate_options(TrainOptions(engine="module", device="gpu", **kw))
        validate_options(TrainOptions(model="resnet18", device="gpu", **kw))
        assert uses_lr_schedule(TrainOptions(**kw))
    check_fused_engine_options(TrainOptions(engine="fused"), fused=True)
    for bad in (dict(lr_schedule="exp"), dict(warmup_steps=-1), dict(lr_schedule="step")):
        with pytest.raises(ValueError):
            validate_options(TrainOptions(**bad))
    # the default flags construct no schedule: FusedSGD takes lr by value
    assert not uses_lr_schedule(TrainOptions()) and build_lr_schedule(TrainOptions(), 3, 10) is None
    # total = epochs * steps per epoch (the ragged flush included), step_size in epochs
    assert optimizer_steps_per_epoch(10, 1) == 10 and optimizer_steps_per_epoch(10, 4) == 3
    assert optimizer_steps_per_epoch(10, 4, max_steps=8) == 2 and optimizer_steps_per_epoch(10, 1, max_steps=50) == 10
    s = build_lr_schedule(TrainOptions(lr=0.2, lr_schedule="step", lr_step_epochs=2, lr_gamma=0.5, warmup_steps=1), 4, 5)
    assert len(s) == 20 and s.values[1].item() == 0.2 and s.values[10].item() == 0.2 and s.values[11].item() == 0.1
    w = build_lr_schedule(TrainOptions(lr=0.2, warmup_steps=4), 2, 5)
    assert w.kind == "none" and len(w) == 10 and w.values[4:].tolist() == [0.2] * 6


def _worker_default(rank, ws, port, ckdir, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import ddp_amd.engine.trainer as tr

    seen = []
    real = tr.FusedSGD

    def spy(*a, **kw):
        seen.append(kw.get("lr_schedule", "absent"))
        return real(*a, **kw)

    tr.FusedSGD = spy
    opts = tr.TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, max_steps=2, num_workers=0,
                           log_every=1000, data="synthetic", save=False)
    tr.ddp_train(rank, ws, 1, 32, opts)
    q.put(seen)


@pytest.mark.slow
def test_default_flags_construct_fused_sgd_without_a_schedule(tmp_path):
    q = mp.get_context("spawn").Queue()
    mp.start_processes(_worker_default, args=(1, free_port(), str(tmp_path / "ck"), q), nprocs=1,
                       start_method="spawn", join=True)
    assert q.get() == [None]
