"""Global-norm gradient clipping fused into FusedSGD (--clip_grad_norm), without a GPU:
the documented summation order of grad_sqnorm_kernel (csrc/kernels/grad_norm.hip) replayed
in float32 against float64 and its a-priori bound, FusedSGD(max_grad_norm=) on the CPU against
torch.nn.utils.clip_grad_norm_ + torch.optim.SGD, the optimizer state, two gloo ranks and
the CLI.  Nothing here is calibrated on the code under test."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ddp_amd.models import SimpleCNN
from ddp_amd.ops import kernel_bounds as kb
from ddp_amd.parallel import free_port

U = kb.U


def mixed(n, seed):
    """Mixed magnitudes: ~1 % of the elements are 10^4 times the rest."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.where(rng.random(n) < 0.01, 100.0, 0.01)).astype(np.float32)


PER_PASS = kb.GN_MAX_BLOCKS * kb.GN_THREADS * kb.GN_QUADS  # quads of one full-grid pass


# ------------------------------------------------------------------ norm order and bound
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1027, 4 * (1024 * 3 + 1) + 2, 4 * (PER_PASS + 1) + 3])
def test_replay_order_is_within_the_bound_and_the_bound_rejects_a_dropped_element(n):
    g = mixed(n, n)
    g[n // 2] = 300.0  # the element the mutation drops: ~ the largest, never negligible
    ref = float((g.astype(np.float64) ** 2).sum())
    b_sum, b_norm, e_coef = kb.sqnorm_bound(n, ref)
    S = kb.replay_sqnorm(g)
    assert abs(float(S) - ref) <= b_sum, (n, float(S), ref, b_sum)
    assert abs(float(np.sqrt(S)) - np.sqrt(ref)) <= b_norm
    # the coefficient, where it clips: torch's fp32 rule on the replayed norm vs float64
    c = 0.25 * np.sqrt(ref)
    coef = kb.clip_coef32(np.sqrt(S), c)
    ref_coef = float(np.float32(c)) / (np.sqrt(ref) + 1e-6)
    assert coef < 1 and abs(float(coef) - ref_coef) <= e_coef * ref_coef
    dropped = kb.replay_sqnorm(g, drop=n // 2)
    assert abs(float(dropped) - ref) > b_sum, "the bound admits a sum with one element missing"


def test_grid_is_a_function_of_n_only_and_the_chain_length_is_as_documented():
    assert kb.grad_norm_blocks(0) == 1 and kb.grad_norm_blocks(4 * 1024) == 1
    assert kb.grad_norm_blocks(4 * 1024 + 4) == 2
    assert kb.grad_norm_blocks(4 * PER_PASS) == kb.GN_MAX_BLOCKS == kb.grad_norm_blocks(1 << 40)
    assert kb.sqnorm_passes(4 * PER_PASS) == 1 and kb.sqnorm_passes(4 * PER_PASS + 4) == 2
    b1, _, _ = kb.sqnorm_bound(4 * PER_PASS, 1.0)
    assert b1 == pytest.approx(27 * U / (1 - 27 * U), rel=1e-12)


def test_coef_rule_is_torchs():
    for norm, c in [(2.0, 1.0), (0.5, 1.0), (0.0, 1.0), (3.7e-3, 1e-2), (1e20, 5.0)]:
        t = (torch.tensor(c, dtype=torch.float32) / (torch.tensor(norm, dtype=torch.float32) + 1e-6)).clamp(max=1.0)
        assert kb.clip_coef32(np.float32(norm), c) == np.float32(t.item())
    assert np.isnan(kb.clip_coef32(np.float32("nan"), 1.0))  # torch.clamp keeps NaN


# ------------------------------------------------------------------------ FusedSGD on CPU
def _batches(k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(8, 1, 28, 28, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(k)]


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("clips", [True, False])
def test_fused_sgd_cpu_matches_clip_grad_norm_and_torch_sgd(momentum, clips):
    """FusedSGD(max_grad_norm=c) against torch.nn.utils.clip_grad_norm_ + torch.optim.SGD run
    in float64 on SimpleCNN's parameters, fed the SAME fp32 gradients every step (ours, from
    forward / backward at our parameters), so the reference's own error is ~1e-16 and the
    difference is the fp32 rounding of our step alone.  Its bound, carried through the steps:

        coefficient   fp32 norm of a float64 sum (u), + 1e-6f, division, the constant: 4 u, and
                      the product g * coef one more: E_d = 6 u |d| (first order terms doubled)
        momentum      E_buf' = m E_buf + E_d + 4 u BUF      (kernel_bounds.sgd_bounds)
        parameter     E_p'   = E_p + lr E_buf' + 6 u P
    """
    from ddp_amd.ops import FusedSGD

    lr, steps = 0.1, 4
    torch.manual_seed(3)
    model = SimpleCNN()
    probe = SimpleCNN()
    probe.load_state_dict(model.state_dict())
    x0, y0 = _batches(1)[0]
    torch.nn.functional.cross_entropy(probe(x0), y0).backward()
    n0 = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in probe.parameters())).item()
    c = 0.3 * n0 if clips else 1e3 * n0
    opt = FusedSGD(model, lr=lr, momentum=momentum, max_grad_norm=c)
    fs = opt.flat
    ref = [torch.nn.Parameter(fs.view(fs.params, n).detach().double().clone()) for n in fs.names]
    topt = torch.optim.SGD(ref, lr=lr, momentum=momentum)
    E_p = torch.zeros(fs.numel, dtype=torch.float64)
    E_buf = torch.zeros(fs.numel, dtype=torch.float64)
    for k, (x, y) in enumerate(_batches(steps)):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        fs.reattach_grads()
        for n, r in zip(fs.names, ref):
            r.grad = fs.view(fs.grads, n).detach().double().clone()
        g64, p64 = fs.grads.double().clone(), fs.params.double().clone()
        m_prev = opt.momentum_buffer.double().clone() if opt.momentum_buffer is not None else torch.zeros_like(g64)
        tnorm = torch.nn.utils.clip_grad_norm_(ref, c)
        topt.step()
        opt.step()
        st = opt.grad_clip_stats()
        ref_coef = min(1.0, c / (tnorm.item() + 1e-6))
        assert abs(st["total_norm"] - tnorm.item()) <= 2 * U * tnorm.item()
        assert abs(st["coef"] - ref_coef) <= 5 * U * ref_coef
        assert (st["coef"] < 1) == clips and st["steps"] == k + 1 and st["clipped"] == (k + 1 if clips else 0)
        d = (g64 * ref_coef).abs()
        E_d = 6 * U * d
        if momentum:
            bp, bb = kb.sgd_bounds(p64, d, m_prev, lr, momentum, 0.0, 0.0, False, k == 0)
            E_buf = (momentum * E_buf if k else 0) + E_d + bb
        else:
            bp, _ = kb.sgd_bounds(p64, d, None, lr, 0.0, 0.0, 0.0, False, k == 0)
            E_buf = E_d
        E_p = E_p + lr * E_buf + bp
        for n, r in zip(fs.names, ref):
            err = (fs.view(fs.params, n).detach().double() - r.detach()).abs()
            bound = fs.view(E_p, n)
            assert bool((err <= bound).all()), (k, n, (err / (bound + 1e-300)).max().item())
    # the padding between parameters carries no gradient: the flat norm is the model's norm
    mask = torch.ones(fs.numel, dtype=torch.bool)
    for n in fs.names:
        mask[fs.offsets[n]:fs.offsets[n] + fs.numels[n]] = False
    assert mask.any() and not fs.grads[mask].any()


def test_max_grad_norm_must_be_positive():
    from ddp_amd.ops import FusedSGD

    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            FusedSGD(SimpleCNN(), lr=0.1, max_grad_norm=bad)
    assert FusedSGD(SimpleCNN(), lr=0.1).grad_clip_stats() is None


# ------------------------------------------------------------------------ optimizer state
def test_state_dict_is_unchanged_by_clipping_and_load_keeps_the_constructors_setting():
    from ddp_amd.ops import FusedSGD

    def run(max_grad_norm):
        torch.manual_seed(5)
        m = SimpleCNN()
        o = FusedSGD(m, lr=0.1, momentum=0.9, max_grad_norm=max_grad_norm)
        for x, y in _batches(2):
            o.zero_grad()
            torch.nn.functional.cross_entropy(m(x), y).backward()
            o.step()
        return m, o

    _, plain = run(None)
    _, huge = run(1e30)  # never clips: coef == 1, so the same updates bit for bit
    a, b = plain.state_dict(), huge.state_dict()
    assert a["param_groups"] == b["param_groups"] and sorted(a["state"]) == sorted(b["state"])
    assert list(a["param_groups"][0]) == list(b["param_groups"][0])
    for i in a["state"]:
        assert list(a["state"][i]) == list(b["state"][i]) == ["momentum_buffer"]
        assert torch.equal(a["state"][i]["momentum_buffer"], b["state"][i]["momentum_buffer"])
    _, clipped = run(1e-3)
    sd = clipped.state_dict()
    assert list(sd) == list(a) and list(sd["param_groups"][0]) == list(a["param_groups"][0])
    # save -> load: clipping follows the constructor of the optimizer that loads
    fresh_off = FusedSGD(SimpleCNN(), lr=0.1, momentum=0.9)
    fresh_off.load_state_dict(sd)
    assert fresh_off.max_grad_norm is None and fresh_off.grad_clip_stats() is None
    fresh_on = FusedSGD(SimpleCNN(), lr=0.1, momentum=0.9, max_grad_norm=0.5)
    fresh_on.load_state_dict(plain.state_dict())
    assert fresh_on.max_grad_norm == 0.5
    assert fresh_on.state_dict()["param_groups"] == a["param_groups"]


# ------------------------------------------------------------------------------ two ranks
def _worker_ddp_clip(rank, ws, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    from torch.nn.parallel import DistributedDataParallel as TorchDDP

    from ddp_amd.models import reference_simple_cnn
    from ddp_amd.ops import FusedSGD
    from ddp_amd.parallel import DistributedDataParallel

    torch.manual_seed(100 + rank)
    ours, ref = SimpleCNN(), reference_simple_cnn()
    if rank == 0:
        ref.load_state_dict(ours.state_dict())
    ddp, tddp = DistributedDataParallel(ours), TorchDDP(ref)
    g = torch.Generator().manual_seed(rank)
    x = torch.rand(6, 1, 28, 28, generator=g)
    y = torch.randint(0, 10, (6,), generator=g)
    c = 0.05  # far below the first steps' norm (~1): every step clips
    opt = FusedSGD(ours, lr=0.1, max_grad_norm=c)
    topt = torch.optim.SGD(ref.parameters(), lr=0.1)
    rows = []
    for _ in range(2):
        opt.zero_grad()
        topt.zero_grad()
        torch.nn.functional.cross_entropy(ddp(x), y).backward()
        torch.nn.functional.cross_entropy(tddp(x), y).backward()
        tnorm = torch.nn.utils.clip_grad_norm_(ref.parameters(), c).item()
        opt.step()
        topt.step()
        st = opt.grad_clip_stats()
        g64 = opt.flat.grads.double()
        rows.append((st["total_norm"], st["coef"], tnorm, g64.square().sum().sqrt().item()))
    sd_ours, sd_ref = ours.state_dict(), ref.state_dict()
    err = max((sd_ours[k] - sd_ref[k]).abs().max().item() for k in sd_ref)
    q.put((rank, err, rows, opt.grad_clip_stats()["clipped"]))
    dist.destroy_process_group()


@pytest.mark.slow
def test_two_rank_ddp_clips_the_all_reduced_gradient_like_torch_ddp():
    """Pattern of test_ddp_cpu.py::test_ddp_matches_torch_ddp_gloo with clipping on both
    sides.  The coefficient and norm are bitwise equal across the ranks (the norm is taken of
    the all-reduced gradient); the norm is the float64 norm of this rank's flat gradient to
    2 u (fp32 rounding of a float64 sum) and torch DDP's clip_grad_norm_ result to 1e-5
    relative (two fp32 backward implementations and torch's own fp32 norm: the agreement that
    pattern test asks of the parameters).  Parameters: that test's 1e-5 at the same lr and
    steps - clipping only shrinks each update (coef <= 1), so the same bound holds."""
    ws = 2
    q = mp.get_context("spawn").Queue()
    mp.start_processes(_worker_ddp_clip, args=(ws, free_port(), q), nprocs=ws, start_method="spawn", join=True)
    res = sorted(q.get() for _ in range(ws))
    (_, err0, rows0, cl0), (_, err1, rows1, cl1) = res
    assert cl0 == cl1 == 2
    for r0, r1 in zip(rows0, rows1):
        assert r0[0] == r1[0] and r0[1] == r1[1], "ranks derived different norms / coefficients"
        assert r0[3] == r1[3], "the all-reduced gradients differ between the ranks"
        assert abs(r0[0] - r0[3]) <= 2 * U * r0[3]
        assert abs(r0[0] - r0[2]) <= 1e-5 * r0[2]
        assert r0[1] < 1
    assert rows0[0][0] != rows0[1][0]  # (the two steps have different norms)
    assert err0 < 1e-5 and err1 < 1e-5, (err0, err1)


# ------------------------------------------------------------------------------------ CLI
def test_cli_fused_engine_refuses_clipping_and_names_the_module_engine():
    import train_ddp
    from ddp_amd.engine.trainer import TrainOptions, check_fused_engine_options, validate_options

    a = train_ddp.parse_args(["--clip_grad_norm", "1.0", "--engine", "fused", "--device", "gpu"])
    assert a.clip_grad_norm == 1.0 and train_ddp.parse_args([]).clip_grad_norm == 0.0
    with pytest.raises(ValueError, match="--engine module"):
        train_ddp.main(["--clip_grad_norm", "1.0", "--engine", "fused", "--device", "gpu"])
    with pytest.raises(ValueError, match="--engine module"):  # what every rank checks once it knows its device
        check_fused_engine_options(TrainOptions(clip_grad_norm=1.0, engine="fused"), fused=True)
    check_fused_engine_options(TrainOptions(clip_grad_norm=1.0, engine="fused"), fused=False)  # the CPU path
    validate_options(TrainOptions(clip_grad_norm=1.0, engine="module", device="gpu"))
    validate_options(TrainOptions(clip_grad_norm=1.0, model="resnet18", device="gpu"))
    with pytest.raises(ValueError):
        validate_options(TrainOptions(clip_grad_norm=-1.0))


def _worker_cli_train(rank, ws, port, ckdir, metrics, clip):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import TrainOptions, ddp_train

    opts = TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, max_steps=3, num_workers=0,
                        log_every=1, data="synthetic", metrics_json=metrics, clip_grad_norm=clip, lr=0.1)
    ddp_train(rank, ws, 2, 32, opts)


@pytest.mark.slow
def test_cpu_trainer_clips_and_records_grad_norm(tmp_path, capfd):
    ck, metrics = str(tmp_path / "ck"), str(tmp_path / "m.jsonl")
    mp.start_processes(_worker_cli_train, args=(1, free_port(), ck, metrics, 0.05), nprocs=1,
                       start_method="spawn", join=True)
    out = capfd.readouterr().out
    assert "Epoch 0 | Batch 0 | Loss:" in out  # the reference's log line, verbatim
    recs = [json.loads(ln) for ln in open(metrics)]
    assert len(recs) == 2
    for i, rec in enumerate(recs):
        assert rec["grad_norm"] > 0.05 and np.isfinite(rec["grad_norm"])
        assert rec["clipped_steps"] == 3 * (i + 1)  # every step of an untrained model clips at 0.05
    assert os.path.exists(os.path.join(ck, "epoch_1.pt"))
