"""Label smoothing (``--label_smoothing``, ``CrossEntropyLoss(label_smoothing=)``) without a GPU:
the float64 references against torch, the a-priori bounds of the SMOOTH kernel builds held
against a float32 emulation of the kernels' order and against wrong kernels, the CPU module,
the binding's range check, the CLI and the evaluation.  tests/label_smoothing_cases.py holds
the inputs, the bounds and the emulation; tests/test_label_smoothing_gpu.py holds the kernels
to the same bounds.  Nothing here is calibrated on the code under test.

Semantics (torch's): target = (1 - e) onehot(y) + e / C over all C classes, so

    loss_row  = logsumexp(x) - (1 - e) x_y - (e / C) sum_c x_c
    dlogits_c = (softmax_c - (1 - e) [c == y] - e / C) g

The kernels (csrc/kernels/xent.hip xent_wave_rows_kernel<true> and xent_kernel<true>, one row
body in csrc/kernels/xent_body.h) get keep = fl(1 - e) and ec = fl(e / C) by value (one rounding each; e is the
float32 the binding narrows the double to, in the reference too) and evaluate, with mx the row
maximum, se = sum exp(x_c - mx), S = sum_c (x_c - mx) over the C valid classes (per lane in
class order, then wave_sum: at most M - 1 + 6 additions on any path, M = ceil(C / 64)):

    d    = ((p - keep [c == y]) - ec) g,              p = exp(x_c - mx) / se
    loss = log(se) - fma(ec, S, keep (x_y - mx))

Bounds, u = 2**-24, extending those of tests/test_resnet_ops_elementwise_gpu.py::run_xent
(D = max |x - mx| of the row, A = sum_c |x_c - mx|, p the float64 softmax):

dlogits.  run_xent's g (p (2 D + 64) u + 2 u) covers p, one subtraction and the product with g.
Smoothing adds three roundings, each of a value of magnitude at most 1: keep (an error
u keep <= u at the label), ec (u e / C <= u on every element) and the second subtraction
(u |p - keep [c == y] - ec| <= u):

    |d - ref| <= g (p (2 D + 64) u + 2 u + 3 u)

loss.  run_xent's (D + 64) u max(1, |ref_row|) per row covers x - mx, the exponentials, the sum,
the logarithm and the final subtraction (log se <= ref_row still holds: the subtracted bracket
is <= 0).  Smoothing adds, per row: keep (x_y - mx) - keep's rounding and the product's, each
u keep |x_y - mx|; S - every term's subtraction and at most M + 5 additions, each relative to
a partial sum of magnitude <= A: (M + 6) u A to first order, (M + 8) u A taken; ec's rounding,
u (e / C) A; and the fma's one rounding, u (keep |x_y - mx| + (e / C) A):

    |loss - ref| <= mean over rows of [(D + 64) u max(1, |ref_row|)
                                       + u (3 keep |x_y - mx| + (M + 10) (e / C) A)]

The emulation stays inside both at every shape and e; each wrong kernel leaves at least one.
"""
import json
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import label_smoothing_cases as LS
from ddp_amd.ops import CrossEntropyLoss
from ddp_amd.ops import reference as R
from ddp_amd.parallel import free_port


# ---------------------------------------------------------------------------- references
@pytest.mark.parametrize("B,C", LS.SHAPES)
@pytest.mark.parametrize("eps", LS.EPSILONS)
def test_float64_references_match_torch_double(B, C, eps):
    lg, lab = LS.xent_inputs(B, C)
    xr = lg.double().requires_grad_(True)
    ref = F.cross_entropy(xr, lab, label_smoothing=eps)
    ref.backward()
    loss, dl = R.xent64(lg, lab, label_smoothing=eps)
    torch.testing.assert_close(loss, ref.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dl, xr.grad, rtol=1e-12, atol=1e-15)
    rows, p = R.xent_rows64(lg, lab, eps)
    torch.testing.assert_close(rows, F.cross_entropy(lg.double(), lab, reduction="none", label_smoothing=eps),
                               rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(p, torch.softmax(lg.double(), 1), rtol=1e-12, atol=1e-300)
    _, dl3 = R.xent64(lg, lab, gscale=0.25, label_smoothing=eps)
    torch.testing.assert_close(dl3, xr.grad * B * 0.25, rtol=1e-12, atol=1e-15)
    # the float32 step reference's loss (the SimpleCNN step oracles use it)
    l32, d32 = R.cross_entropy(lg.double(), lab, eps)
    torch.testing.assert_close(l32, ref.detach(), rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(d32, xr.grad, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("B,C", LS.SHAPES)
def test_references_at_zero_are_todays_bit_for_bit(B, C):
    """The references as they were before they took the argument, written out here."""
    lg, lab = LS.xent_inputs(B, C)
    x = lg.double()
    z = x - x.max(1, keepdim=True).values
    lse = z.exp().sum(1).log()
    rows0, p0 = lse - z[torch.arange(B), lab], (z - lse[:, None]).exp()
    d0 = p0.clone()
    d0[torch.arange(B), lab] -= 1.0
    for kw in ({}, {"label_smoothing": 0.0}):
        rows, p = R.xent_rows64(lg, lab, **kw)
        loss, dl = R.xent64(lg, lab, **kw)
        assert torch.equal(rows, rows0) and torch.equal(p, p0)
        assert torch.equal(loss, rows0.mean()) and torch.equal(dl, d0 * (1.0 / B))
    lp = torch.log_softmax(lg, dim=1)
    dd = lp.exp()
    dd[torch.arange(B), lab] -= 1.0
    for kw in ({}, {"label_smoothing": 0.0}):
        l1, d1 = R.cross_entropy(lg, lab, **kw)
        assert torch.equal(l1, F.nll_loss(lp, lab)) and torch.equal(d1, dd / B)


# --------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("B,C", LS.SHAPES + [(4, 1000), (7, 1024)])
@pytest.mark.parametrize("eps", [0.1, 0.5, 1.0])
def test_emulation_of_the_kernels_order_is_within_the_bounds(B, C, eps):
    lg, lab = LS.xent_inputs(B, C)
    e, g = LS.f32(eps), LS.f32(1.0 / B)
    loss_ref, dl_ref, bl, bd = LS.bounds(lg, lab, e, g)
    loss, dl = LS.emulate(lg, lab, e, g)
    ok_d, rd = LS.within(dl, dl_ref, bd)
    ok_l, rl = LS.within(loss, loss_ref, bl)
    print(f"CPU_RATIO label_smoothing {(B, C, eps)} dlogits {rd:.4f} loss {rl:.4f}")
    assert ok_d and ok_l, (rd, rl)
    # every row's gradient sums to zero within the sum of its elements' bounds
    assert bool((dl.double().sum(1).abs() <= bd.sum(1)).all())


# logit_magnitude at e = 0.1 only: its error is the rounding of keep x_y, ec sum x and mx + log se
# at the logits' magnitude (the rows offset by 1e4: half an ulp of 1e4 is 8192 u each), and the
# mean's bound is dominated by the spread-60 rows' (D + 64) |ref_row| u of about 4000 u each.  At
# e = 1 keep is 0, the largest of those roundings is gone and what is left need not leave the bound.
WRONG = [(v, e) for v in ("other_classes", "grad_only", "loss_only", "all_slots", "all_slots_zero") for e in (0.1, 1.0)]
WRONG.append(("logit_magnitude", 0.1))


@pytest.mark.parametrize("variant,eps", WRONG)
@pytest.mark.parametrize("B,C", [(7, 10), (1, 65), (9, 127)])
def test_the_bounds_reject_wrong_kernels(variant, B, C, eps):
    lg, lab = LS.xent_inputs(B, C)
    e, g = LS.f32(eps), LS.f32(1.0 / B)
    loss_ref, dl_ref, bl, bd = LS.bounds(lg, lab, e, g)
    loss, dl = LS.emulate(lg, lab, e, g, variant)
    ok_d, rd = LS.within(dl, dl_ref, bd)
    ok_l, rl = LS.within(loss, loss_ref, bl)
    print(f"CPU_RATIO label_smoothing wrong {variant} {(B, C, eps)} dlogits {rd:.3g} loss {rl:.3g}")
    assert not (ok_d and ok_l), f"the bounds admit {variant}: {rd:.3g} {rl:.3g}"
    if variant in ("grad_only", "all_slots", "all_slots_zero", "logit_magnitude"):
        assert ok_d and not ok_l  # these touch the loss alone
    if variant == "loss_only":
        assert ok_l and not ok_d


# ------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("eps", LS.EPSILONS)
def test_cross_entropy_loss_on_cpu_is_torchs_criterion(eps):
    lg, lab = LS.xent_inputs(9, 127)
    a = lg.clone().requires_grad_(True)
    b = lg.clone().requires_grad_(True)
    ours = CrossEntropyLoss(label_smoothing=eps)
    la, lb = ours(a, lab), torch.nn.CrossEntropyLoss(label_smoothing=eps)(b, lab)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert ours.label_smoothing == eps and CrossEntropyLoss().label_smoothing == 0.0
    assert torch.equal(CrossEntropyLoss()(lg, lab), F.cross_entropy(lg, lab))


@pytest.mark.parametrize("bad", [-0.1, 1.5, math.nan, math.inf])
def test_out_of_range_values_raise(bad):
    from ddp_amd.engine.trainer import TrainOptions, validate_options

    with pytest.raises(ValueError):
        CrossEntropyLoss(label_smoothing=bad)
    with pytest.raises(ValueError):
        validate_options(TrainOptions(label_smoothing=bad))


@pytest.mark.parametrize("bad", [-0.1, 1.0000001, math.nan, math.inf])
def test_binding_checks_the_range_before_anything_else(bad):
    from ddp_amd import native

    if not native.available():
        pytest.skip("the native extension is not built")
    C = native.require()
    lg, lab = torch.zeros(2, 10), torch.zeros(2, dtype=torch.long)
    dl, loss = torch.zeros(2, 10), torch.zeros(1)
    with pytest.raises(ValueError, match="label_smoothing"):  # (CPU tensors: no launch is ever reached)
        C.xent(lg, 1, None, lab, None, dl, loss, None, 0.5, 0.0, label_smoothing=bad)


# ------------------------------------------------------------------------------------ CLI
def test_cli_fused_engine_refuses_the_flag_and_names_the_module_engine():
    import train_ddp
    from ddp_amd.engine.trainer import TrainOptions, check_fused_engine_options, validate_options

    a = train_ddp.parse_args(["--label_smoothing", "0.1", "--engine", "fused", "--device", "gpu"])
    assert a.label_smoothing == 0.1
    with pytest.raises(ValueError, match="--engine module"):
        train_ddp.main(["--label_smoothing", "0.1", "--engine", "fused", "--device", "gpu"])
    with pytest.raises(ValueError, match="--engine module"):  # what every rank checks once it knows its device
        check_fused_engine_options(TrainOptions(label_smoothing=0.1, engine="fused"), fused=True)
    check_fused_engine_options(TrainOptions(label_smoothing=0.1, engine="fused"), fused=False)  # the CPU path
    validate_options(TrainOptions(label_smoothing=0.1, engine="module", device="gpu"))
    validate_options(TrainOptions(label_smoothing=0.1, model="resnet18", device="gpu", graph_module=True))
    validate_options(TrainOptions(label_smoothing=1.0, grad_accum=2, device="cpu"))


def test_default_flags_build_the_plain_criterion(monkeypatch):
    """--label_smoothing reaches trainer.py's loss_fn; the default flags build CrossEntropyLoss()
    with e = 0 (ddp_train is stopped right after it built the criterion)."""
    import train_ddp
    from ddp_amd.engine import trainer

    assert train_ddp.parse_args([]).label_smoothing == 0.0 and trainer.TrainOptions().label_smoothing == 0.0
    seen = []

    class Stop(Exception):
        pass

    class Spy(CrossEntropyLoss):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append(self.label_smoothing)
            raise Stop

    monkeypatch.setattr(trainer, "CrossEntropyLoss", Spy)
    monkeypatch.setattr(train_ddp, "launch", lambda fn, ws, args: fn(0, ws, *args))
    monkeypatch.delenv("MASTER_PORT", raising=False)
    for flags in ([], ["--label_smoothing", "0.25"]):
        try:
            with pytest.raises(Stop):
                train_ddp.main(["--device", "cpu", "--data", "synthetic", "--num_workers", "0", "--no_save",
                                "--world_size", "1"] + flags)
        finally:
            if dist.is_initialized():
                dist.destroy_process_group()
    assert seen == [0.0, 0.25]


def _worker_cli_vs_torch(rank, ws, port, port2, ckdir, metrics, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import train_ddp
    from ddp_amd.data import get_dataloader
    from ddp_amd.engine import trainer
    from ddp_amd.models import SimpleCNN, reference_simple_cnn

    # the CLI's own path from the flags to the options, then this rank's ddp_train
    box = {}
    train_ddp.launch = lambda fn, n, args: box.update(fn=fn, n=n, args=args)
    train_ddp.main(["--device", "cpu", "--backend", "gloo", "--label_smoothing", "0.1", "--world_size", str(ws),
                    "--epochs", "1", "--batch_size", "32", "--max_steps", "3", "--lr", "0.1", "--data", "synthetic",
                    "--num_workers", "0", "--checkpoint_dir", ckdir, "--log_every", "1", "--metrics_json", metrics])
    assert box["fn"] is trainer.ddp_train and box["n"] == ws
    model = box["fn"](rank, ws, *box["args"])
    # a plain torch DDP loop over the same batches with torch's criterion
    os.environ["MASTER_PORT"] = str(port2)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    from torch.nn.parallel import DistributedDataParallel as TorchDDP

    torch.manual_seed(0)  # TrainOptions.seed: the trainer seeds, then builds its model
    init = {k: v.clone() for k, v in SimpleCNN().state_dict().items()}
    ref = reference_simple_cnn()
    ref.load_state_dict(init)
    tddp = TorchDDP(ref)
    topt = torch.optim.SGD(ref.parameters(), lr=0.1)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    loader, sampler = get_dataloader(32, ws, rank, source="synthetic", num_workers=0)
    sampler.set_epoch(0)
    losses = []
    for i, (x, y) in enumerate(loader):
        if i == 3:
            break
        topt.zero_grad()
        loss = crit(tddp(x), y)
        loss.backward()
        topt.step()
        losses.append(loss.item())
    sd_ours, sd_ref = model.state_dict(), ref.state_dict()
    err = max((sd_ours[k] - sd_ref[k]).abs().max().item() for k in sd_ref)
    moved = max((sd_ref[k] - init[k]).abs().max().item() for k in sd_ref)
    q.put((rank, err, moved, losses))
    dist.destroy_process_group()


@pytest.mark.slow
def test_two_rank_cpu_cli_run_ends_at_torch_ddps_parameters(tmp_path, capfd):
    """Tolerance: tests/test_ddp_cpu.py::test_ddp_matches_torch_ddp_gloo's 1e-5 on the parameters
    at the same learning rate (two fp32 backward implementations), here after 3 steps."""
    ws = 2
    ck, metrics = str(tmp_path / "ck"), str(tmp_path / "m.jsonl")
    q = mp.get_context("spawn").Queue()
    mp.start_processes(_worker_cli_vs_torch, args=(ws, free_port(), free_port(), ck, metrics, q), nprocs=ws,
                       start_method="spawn", join=True)
    res = sorted(q.get() for _ in range(ws))
    for rank, err, moved, _ in res:
        assert moved > 1e-3  # (the run trained)
        assert err < 1e-5, f"rank {rank} ends {err} away from the torch DDP loop"
    out = capfd.readouterr().out
    # the logged loss is the smoothed one: rank 0's torch losses, as the log line rounds them
    for i, lv in enumerate(res[0][3]):
        line = next(ln for ln in out.splitlines() if ln.startswith(f"Epoch 0 | Batch {i} | Loss:"))
        assert abs(float(line.rsplit(":", 1)[1]) - lv) <= 1e-4 + 5e-5, (line, lv)
    recs = [json.loads(ln) for ln in open(metrics)]
    assert len(recs) == 1 and recs[0]["label_smoothing"] == 0.1


# ------------------------------------------------------------------------------ evaluation
def test_evaluation_does_not_depend_on_the_training_flag():
    """run_eval of a fixed model: the plain cross-entropy whatever --label_smoothing trains with."""
    from ddp_amd.data import DeviceMNIST, synthetic_mnist
    from ddp_amd.engine.trainer import TrainOptions, run_eval
    from ddp_amd.models import SimpleCNN

    torch.manual_seed(3)
    model = SimpleCNN()
    with torch.no_grad():
        model.fl.weight.mul_(100.0)  # peaked logits: the smoothed and the plain loss differ
    imgs, labels = synthetic_mnist(37)
    data = DeviceMNIST(imgs, labels, "cpu")
    res = [run_eval(model, None, data, torch.device("cpu"), TrainOptions(label_smoothing=e, eval_batch_size=16,
                                                                          device="cpu"), 0, 1, False)
           for e in (0.0, 0.1, 1.0)]
    with torch.no_grad():
        lg = model(imgs.float().div(255).unsqueeze(1))
    want = F.cross_entropy(lg.double(), labels, reduction="sum").item()
    for r in res:
        assert (r.correct, r.count, r.loss_sum) == (res[0].correct, res[0].count, res[0].loss_sum)
        assert torch.equal(r.pred, res[0].pred) and torch.equal(r.loss, res[0].loss)
        assert abs(r.loss_sum - want) <= 1e-4 * want
    smoothed = F.cross_entropy(lg.double(), labels, reduction="sum", label_smoothing=0.1).item()
    assert abs(smoothed - want) > 10 * 1e-4 * want  # (the tolerance above tells the two losses apart)


def test_metrics_record_gains_the_key_only_when_non_zero(tmp_path):
    from ddp_amd.engine.trainer import TrainOptions, _record_metrics

    path = str(tmp_path / "m.jsonl")
    _record_metrics(TrainOptions(metrics_json=path), 0, 1, 0, 3, 32, 1.0, 96)
    _record_metrics(TrainOptions(metrics_json=path, label_smoothing=0.1), 0, 1, 0, 3, 32, 1.0, 96)
    a, b = [json.loads(ln) for ln in open(path)]
    assert "label_smoothing" not in a and b["label_smoothing"] == 0.1
    assert {k: v for k, v in b.items() if k != "label_smoothing"} == a
