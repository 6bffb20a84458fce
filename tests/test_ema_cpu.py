"""The weight EMA (ddp_amd.ops.ema, --ema_decay / --ema_warmup / --eval_ema) without a GPU: the
element bound of one update, derived here; the warm-up decay table against its closed form;
``applied()``; the checkpoint entry; crash and resume over two gloo ranks; the flag checks.
Nothing here is calibrated on the code under test.

The element bound.  With fp32 inputs e, p and the fp32 ``om``, ``ref = e + om (p - e)`` in float64
(exact to ~2^-53, negligible).  The update is one fp32 subtraction, ``d = fl(p - e)`` with
``|d - (p - e)| <= u |p - e|`` (u = 2^-24), then one fused multiply-add, ``fl(e + om d)``: the
subtraction's error reaches the result scaled by om, and the final rounding adds at most
``u |result|``, so

    |got - ref| <= u (om |p - e| + |ref|) (1 + 2^-20)

the last factor covering the second-order terms (|result| against |ref|).  A form that rounds
``(1 - om) e`` and ``om p`` separately carries ``u (|e| + ...)`` instead, which the bound refuses
whenever p is close to e - the case an EMA lives in."""
import os
import struct

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from ddp_amd.models import SimpleCNN
from ddp_amd.models.layers import flat_space
from ddp_amd.ops import FusedSGD, WeightEMA
from ddp_amd.ops.ema import MAX_TABLE, warmup_table
from ddp_amd.parallel import free_port

U = 2.0 ** -24


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def ema_bound(e32, p32, om32):
    """(ref, bound) of one update in float64, from the fp32 inputs (numpy arrays) and the fp32 om."""
    e, p = e32.astype(np.float64), p32.astype(np.float64)
    ref = e + float(om32) * (p - e)
    return ref, U * (float(om32) * np.abs(p - e) + np.abs(ref)) * (1 + 2.0 ** -20)


def mixed_inputs(n, seed):
    """Normal-range values of mixed sign and magnitude (2^-20 .. 2^20)."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(n, generator=g, dtype=torch.float64) * 40 - 20)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


# --------------------------------------------------------------------------- the element bound
@pytest.mark.parametrize("warmup", [False, True])
def test_cpu_update_meets_the_element_bound_over_50_updates(warmup):
    """Per element and per update, against the float64 reference of that update's own inputs.
    The parameters move between updates: close to the average (the common case), far from it,
    and across zero."""
    torch.manual_seed(0)
    model = SimpleCNN()
    ema = WeightEMA(model, decay=0.99, warmup=warmup)
    fs = ema.flat
    n = fs.numel
    live = torch.zeros(n, dtype=torch.bool)
    for name in fs.names:
        live[fs.offsets[name]:fs.offsets[name] + fs.numels[name]] = True
    with torch.no_grad():
        fs.params[live] = mixed_inputs(int(live.sum()), 1)
    ema.reset()
    g = torch.Generator().manual_seed(2)
    worst = 0.0
    for k in range(50):
        with torch.no_grad():
            if k % 3 == 0:  # a small relative step, as an optimizer takes
                fs.params.mul_(1 + 1e-3 * torch.randn(n, generator=g))
            elif k % 3 == 1:  # unrelated values of mixed sign and magnitude
                fs.params[live] = mixed_inputs(int(live.sum()), 100 + k)
            else:
                fs.params.neg_()
        e0, p0 = ema.params.numpy().copy(), fs.params.detach().numpy().copy()
        om = ema.om_at(k)
        assert om == f32(1 - (min(0.99, (1 + k) / (10 + k)) if warmup else 0.99))
        ema.update()
        ref, bound = ema_bound(e0, p0, om)
        err = np.abs(ema.params.numpy().astype(np.float64) - ref)
        assert np.all(err <= bound), (k, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    assert ema.num_updates() == 50
    assert not ema.params[~live].any(), "alignment padding stays zero"
    print(f"EMA_CPU_RATIO warmup={warmup} worst err/bound = {worst:.3f}")


def test_two_product_form_fails_the_bound_on_the_same_inputs():
    """``fl(fl(1 - om) e) + fl(om p)`` rounds two products of the size of e: with p within 1e-3
    of e (an optimizer step) its error is ~u |e|, far above u (om |p - e| + |ref|)'s first term
    and - over thousands of elements - above the whole bound for some of them.  The update
    under test meets the bound on exactly these inputs."""
    n = 4096
    e = mixed_inputs(n, 7)
    p = (e.double() * (1 + 1e-3 * torch.randn(n, generator=torch.Generator().manual_seed(8), dtype=torch.float64))).float()
    om = f32(1 - 0.9999)
    ref, bound = ema_bound(e.numpy(), p.numpy(), om)
    two = (torch.tensor(f32(1 - om)) * e + torch.tensor(om) * p).numpy().astype(np.float64)
    assert np.any(np.abs(two - ref) > bound), "the two-product form should break the bound"
    # the same inputs through the class
    m = torch.nn.Linear(64, 64, bias=False)
    ema = WeightEMA(m, decay=0.9999)
    with torch.no_grad():
        ema.params[:n].copy_(e)
        ema.flat.params[:n].copy_(p)
    ema.update()
    assert np.all(np.abs(ema.params[:n].numpy().astype(np.float64) - ref) <= bound)


# ------------------------------------------------------------------------- the warm-up table
@pytest.mark.parametrize("decay", [0.5, 0.9, 0.99, 0.999, 0.9999])
def test_warmup_table_entries_length_and_hold(decay):
    tab = warmup_table(decay)
    assert tab.dtype == torch.float32 and tab.dim() == 1
    want = [f32(1 - min(decay, (1 + k) / (10 + k))) for k in range(tab.numel())]
    assert tab.tolist() == want
    # it ends at the first k whose warm-up term reaches the decay
    K = tab.numel() - 1
    assert (1 + K) / (10 + K) >= decay and (K == 0 or K / (9 + K) < decay)
    assert tab[-1].item() == f32(1 - decay)
    # the last entry holds past the end
    ema = WeightEMA(torch.nn.Linear(4, 4), decay=decay, warmup=True)
    assert [ema.om_at(k) for k in (K, K + 1, 10 * K + 7)] == [f32(1 - decay)] * 3
    assert ema.om_at(0) == f32(1 - min(decay, 0.1))


def test_warmup_table_cap_refuses():
    assert MAX_TABLE == 1 << 22
    with pytest.raises(ValueError, match="table"):
        warmup_table(0.999999)  # ~9e6 updates
    with pytest.raises(ValueError, match="table"):
        WeightEMA(torch.nn.Linear(4, 4), decay=0.999999, warmup=True)
    WeightEMA(torch.nn.Linear(4, 4), decay=0.999999)  # a constant decay needs no table
    n = warmup_table(0.99).numel()
    assert 880 < n < 900 and warmup_table(0.99, max_len=n).numel() == n
    with pytest.raises(ValueError, match="table"):
        warmup_table(0.99, max_len=n - 1)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            WeightEMA(torch.nn.Linear(4, 4), decay=bad)


# --------------------------------------------------------------------------------- applied()
def _trained(model_fn, steps=4, **ema_kw):
    torch.manual_seed(0)
    model = model_fn()
    opt = FusedSGD(model, lr=0.05, momentum=0.9)
    ema = WeightEMA(model, **ema_kw)
    opt.attach_ema(ema)
    x = torch.rand(8, 1, 28, 28)
    y = torch.randint(0, 10, (8,))
    for _ in range(steps):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        opt.step()
    return model, opt, ema, x


def test_applied_is_the_averaged_model_and_restores_bitwise():
    model, opt, ema, x = _trained(SimpleCNN, decay=0.9, warmup=True)
    assert ema.num_updates() == opt.steps == 4
    assert not torch.equal(ema.params, ema.flat.params)
    fresh = SimpleCNN()
    fresh.load_state_dict(ema.state_dict()["model"])
    flat_space(fresh)  # the same storage layout: the CPU GEMMs' summation order follows the alignment
    fs = ema.flat
    before = (fs.params.clone(), fs.grads.clone(), ema.params.clone(),
              {k: v.clone() for k, v in model.state_dict().items()})
    with torch.no_grad():
        live_out = model(x)
        with ema.applied() as m:
            assert m is model
            assert torch.equal(fs.params, before[2]), "inside, the parameters hold the EMA's bits"
            inside = model(x)
            with pytest.raises(RuntimeError):  # nested use
                with ema.applied():
                    pass
            with pytest.raises(RuntimeError):
                ema.update()
        assert torch.equal(inside, fresh(x))
        assert not torch.equal(inside, live_out)
        assert torch.equal(model(x), live_out)
    assert torch.equal(fs.params, before[0]) and torch.equal(fs.grads, before[1])
    assert torch.equal(ema.params, before[2])
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[3][k]), k
    with ema.applied():  # usable again after the failed nested entry
        pass
    assert torch.equal(fs.params, before[0])


def test_applied_with_batchnorm_uses_the_live_buffers():
    from ddp_amd.models import resnet18

    torch.manual_seed(0)
    model = resnet18(num_classes=10)
    opt = FusedSGD(model, lr=0.05)
    ema = WeightEMA(model, decay=0.5)
    opt.attach_ema(ema)
    x = torch.rand(4, 3, 32, 32)
    y = torch.randint(0, 10, (4,))
    for _ in range(2):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        opt.step()
    model.eval()
    sd = ema.state_dict()["model"]
    live = model.state_dict()
    for k in live:
        if "running_" in k or "num_batches" in k:
            assert torch.equal(sd[k], live[k]), k
    fresh = resnet18(num_classes=10)
    fresh.load_state_dict(sd)
    flat_space(fresh)
    fresh.eval()
    bufs = {k: v.clone() for k, v in model.named_buffers()}
    with torch.no_grad(), ema.applied():
        inside = model(x)
    with torch.no_grad():
        assert torch.equal(inside, fresh(x))
    for k, v in model.named_buffers():
        assert torch.equal(v, bufs[k]), k


def test_set_num_updates_refuses_inside_a_capture(monkeypatch):
    """With a device-resident counter (stood in for by a host tensor here) the write is a copy
    from the host: refused while the current stream is capturing, as set_schedule_step is."""
    ema = WeightEMA(torch.nn.Linear(4, 4), decay=0.9)
    ema._ws = (None, torch.zeros(4, dtype=torch.int32))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    ema.set_num_updates(3)
    assert ema.num_updates() == 3 and ema._ws[1].tolist() == [3, 0, 0, 0]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        ema.set_num_updates(5)
    assert ema.num_updates() == 3


def test_update_only_on_optimizer_steps_and_detach():
    model, opt, ema, _ = _trained(SimpleCNN, steps=3, decay=0.9)
    assert ema.num_updates() == 3
    opt.attach_ema(None)
    opt.step()
    assert ema.num_updates() == 3 and opt.steps == 4
    with pytest.raises(ValueError):
        opt.attach_ema(WeightEMA(SimpleCNN()))
    ema.reset()
    assert ema.num_updates() == 0 and torch.equal(ema.params, ema.flat.params)
    ema.set_num_updates(7)
    assert ema.num_updates() == 7
    with pytest.raises(ValueError):
        ema.set_num_updates(-1)


# -------------------------------------------------------------------------------- checkpoints
def test_checkpoint_has_an_ema_entry_only_with_an_attached_ema(tmp_path):
    from ddp_amd.utils.checkpoint import build_checkpoint, load_checkpoint, save_checkpoint

    model, opt, ema, x = _trained(SimpleCNN, decay=0.99, warmup=True)
    opt.attach_ema(None)
    assert list(build_checkpoint(0, model, opt)) == ["epoch", "model", "optimizer"]
    opt.attach_ema(ema)
    ck = build_checkpoint(0, model, opt)
    assert list(ck) == ["epoch", "model", "optimizer", "ema"]
    assert list(ck["ema"]) == ["decay", "warmup", "num_updates", "model"]
    assert (ck["ema"]["decay"], ck["ema"]["warmup"], ck["ema"]["num_updates"]) == (0.99, True, 4)
    assert list(ck["ema"]["model"]) == list(ck["model"])
    # through a file: the round trip is exact, and a plain model loads the entry
    path = save_checkpoint(str(tmp_path), 0, model, opt)
    saved = load_checkpoint(path)["ema"]
    other = WeightEMA(SimpleCNN(), decay=0.99, warmup=True)
    other.load_state_dict(saved)
    assert torch.equal(other.params, ema.params) and other.num_updates() == 4
    plain = SimpleCNN()
    plain.load_state_dict(saved["model"])
    flat_space(plain)
    with torch.no_grad(), ema.applied():
        assert torch.equal(plain(x), model(x))
    again = other.state_dict()
    assert again["num_updates"] == 4
    for k, v in saved["model"].items():
        if k in dict(other.model.named_parameters()):
            assert torch.equal(again["model"][k], v), k


# ------------------------------------------------------------------------ crash and resume
def _worker_fault(rank, ws, port, ckdir, epochs, fault):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import TrainOptions, ddp_train

    opts = TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, max_steps=12, num_workers=0,
                        log_every=1000, data="synthetic", fault=fault, momentum=0.9, lr=0.05,
                        ema_decay=0.99, ema_warmup=True, verify_replicas=True)
    ddp_train(rank, ws, epochs, 32, opts)


@pytest.mark.slow
def test_fault_then_resume_is_byte_identical_with_an_ema(tmp_path, capfd):
    """test_ddp_cpu.py::test_fault_then_resume_is_byte_identical with --ema_decay 0.99
    --ema_warmup: a crash in epoch 1, auto-resume (rank 0 loads the "ema" entry, rank 1 receives
    the buffer and the count), and the final checkpoint equals the uninterrupted run's - every
    zip record except the random serialization_id, the "ema" entry included.  --verify_replicas
    hashes the EMA: both ranks' digests are equal after every epoch, or the run raises."""
    import zipfile

    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    mp.start_processes(_worker_fault, args=(2, free_port(), a, 3, None), nprocs=2, start_method="spawn", join=True)
    out = capfd.readouterr().out
    assert out.count("replicas bitwise identical") == 3 and out.count("weight EMA ") == 3
    with pytest.raises(Exception):
        mp.start_processes(_worker_fault, args=(2, free_port(), b, 3, (1, 5, 1)), nprocs=2,
                           start_method="spawn", join=True)
    assert sorted(os.listdir(b)) == ["epoch_0.pt"]
    mp.start_processes(_worker_fault, args=(2, free_port(), b, 3, None), nprocs=2, start_method="spawn", join=True)
    out = capfd.readouterr().out
    assert "Resumed from" in out and "WARNING" not in out
    assert out.count("replicas bitwise identical") == 3  # epoch 0 before the crash, 1 and 2 after the resume
    za, zb = zipfile.ZipFile(os.path.join(a, "epoch_2.pt")), zipfile.ZipFile(os.path.join(b, "epoch_2.pt"))
    diff = [i.filename for i in za.infolist() if za.read(i.filename) != zb.read(i.filename)]
    assert set(diff) <= {"epoch_2/.data/serialization_id"}, diff
    ck = torch.load(os.path.join(b, "epoch_2.pt"), weights_only=True)
    assert ck["ema"]["num_updates"] == 36 and ck["ema"]["warmup"] is True and ck["ema"]["decay"] == 0.99
    assert any(not torch.equal(ck["ema"]["model"][k], ck["model"][k]) for k in ck["model"])


def _worker_restart(rank, ws, port, ckdir, epochs):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import TrainOptions, ddp_train

    opts = TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, max_steps=3, num_workers=0,
                        log_every=1000, data="synthetic", ema_decay=0.0 if epochs == 1 else 0.9)
    ddp_train(rank, ws, epochs, 32, opts)


@pytest.mark.slow
def test_resume_without_an_ema_entry_restarts_the_average(tmp_path, capfd):
    ck = str(tmp_path / "c")
    mp.start_processes(_worker_restart, args=(1, free_port(), ck, 1), nprocs=1, start_method="spawn", join=True)
    assert "ema" not in torch.load(os.path.join(ck, "epoch_0.pt"), weights_only=True)
    capfd.readouterr()
    mp.start_processes(_worker_restart, args=(1, free_port(), ck, 2), nprocs=1, start_method="spawn", join=True)
    out = capfd.readouterr().out
    assert "WARNING: the checkpoint holds no weight EMA" in out
    assert torch.load(os.path.join(ck, "epoch_1.pt"), weights_only=True)["ema"]["num_updates"] == 3


# ------------------------------------------------------------------------------------ flags
def test_flag_checks():
    import train_ddp
    from ddp_amd.engine.trainer import TrainOptions, check_fused_engine_options, validate_options

    d = train_ddp.parse_args([])
    assert (d.ema_decay, d.ema_warmup, d.eval_ema) == (0.0, False, False)
    with pytest.raises(ValueError, match="--engine module"):
        train_ddp.main(["--ema_decay", "0.99", "--engine", "fused", "--device", "gpu"])
    with pytest.raises(ValueError, match="--engine module"):
        check_fused_engine_options(TrainOptions(engine="fused", ema_decay=0.99), fused=True)
    check_fused_engine_options(TrainOptions(engine="fused", ema_decay=0.99), fused=False)  # the CPU path
    check_fused_engine_options(TrainOptions(engine="fused"), fused=True)
    validate_options(TrainOptions(engine="module", device="gpu", ema_decay=0.99, ema_warmup=True))
    validate_options(TrainOptions(model="resnet18", device="gpu", ema_decay=0.99, eval_ema=True, eval_every=1,
                                  eval_size=64))
    with pytest.raises(ValueError, match="--ema_decay"):
        train_ddp.main(["--eval_ema", "--eval_every", "1", "--device", "cpu"])
    with pytest.raises(ValueError, match="--ema_decay"):
        validate_options(TrainOptions(eval_ema=True))
    for bad in (1.0, -0.5, 2.0):
        with pytest.raises(ValueError):
            validate_options(TrainOptions(ema_decay=bad))
