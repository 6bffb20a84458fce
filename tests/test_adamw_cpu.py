"""FusedAdamW on the CPU path: state-dict format, one step against torch.optim.AdamW under a
derived per-element bound, the coefficient table, two ranks over gloo, option errors.

The bound (also asserted for the GPU kernel, tests/test_adamw_gpu.py).  The documented
sequence (csrc/kernels/adamw.hip) is, in fp32 with unit roundoff u = 2^-24,

    p1  = p * decay                    one rounding:            |err| <= u |p decay|
    m'  = m + w1 (d - m)               d - m, the product and the sum round (a fma drops one):
                                       |err| <= u (|d - m| + 2 |m'|) <= 3u (|m| + |g|)
    v'  = b2 v + w2 d d                all terms >= 0; three products and one sum, each term
                                       carries at most (1 + u)^3:   |err| <= 4u v'
    den = sqrt(v') / bc2_sqrt + eps    sqrt halves v's 4u and adds u, the divide and the add
                                       one u each:                  |err| <= 5u den
    q   = m' / den                     |err| <= (3u (|m| + |g|) + 6u |m'|) / den
    p'  = p1 - step_size q             the product and the sum round (a fma drops one):
                                       |err| <= u |p decay| + u |p'| + step_size (|err q| + u |q|)

With |p'| <= |p decay| + step_size |m'| / den this gives, every quantity taken from the float64
evaluation of the same sequence on the same fp32 scalars (first-order terms; the slack of the
integer constants covers the second-order ones),

    |dp| <= u (2 |p decay| + step_size (8 |m'| + 4 (|m| + |g|)) / den)
    |dm| <= 3u (|m| + |g|)
    |dv| <= 4u v'

An unfused fp32 replay of the sequence (every torch op rounds once) stays inside the p bound
at t in {1, 2, 10, 1000, 20000}; three plausible wrong sequences - eps added before the
second-moment correction, no second-moment correction, no first-moment correction - leave it
on more than 40 % of the elements at t in {1, 2, 10}.  Both facts are asserted, so the bound
is neither vacuous nor unreachable.
"""
import os

import pytest
import torch
import torch.multiprocessing as mp

from ddp_amd.ops import FusedAdamW, LRSchedule
from ddp_amd.ops.adamw import _f32, coef_entry, coef_table

U = 2.0 ** -24
N = 200003
LR, WD, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.999, 1e-8


class Vec(torch.nn.Module):
    def __init__(self, n, init=None):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(n) if init is None else init.clone())


def make_inputs(n=N, seed=0, zero_state=False, nzero=1000):
    """p ~ N(0, 1); g = N(0, 1) * 10^U(-10, 2) with the first ``nzero`` entries exactly 0; m of g's
    scale and v of its square's (zero for the first step)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    scale = 10.0 ** (torch.rand(n, generator=gen) * 12 - 10)
    g = torch.randn(n, generator=gen) * scale
    g[:min(nzero, n)] = 0
    if zero_state:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = torch.randn(n, generator=gen) * scale
        v = (torch.randn(n, generator=gen) * scale).square()
    return p, g, m, v


def scalars32(t, lr=LR, wd=WD, b1=B1, b2=B2, eps=EPS):
    """The fp32 scalars of optimizer step t (1-based), as Python floats."""
    decay, step_size, bc2_sqrt, _ = (_f32(x) for x in coef_entry(t - 1, lr, b1, b2, wd))
    return dict(decay=decay, step_size=step_size, bc2_sqrt=bc2_sqrt, w1=_f32(1 - b1), b2=_f32(b2),
                w2=_f32(1 - b2), eps=_f32(eps))


def ref64(p, g, m, v, s, gscale=None, maximize=False):
    """The documented sequence in float64 on the fp32 scalars; returns (p', m', v', bounds)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    d = g if gscale is None else (g.float() * torch.tensor(gscale, dtype=torch.float32)).double()
    if maximize:
        d = -d
    p1 = p * s["decay"]
    m1 = m + s["w1"] * (d - m)
    v1 = s["b2"] * v + s["w2"] * d * d
    den = v1.sqrt() / s["bc2_sqrt"] + s["eps"]
    p2 = p1 - s["step_size"] * (m1 / den)
    bp = U * (2 * p1.abs() + s["step_size"] * (8 * m1.abs() + 4 * (m.abs() + d.abs())) / den)
    bm = 3 * U * (m.abs() + d.abs())
    bv = 4 * U * v1
    return p2, m1, v1, (bp, bm, bv)


def check_bounds(got, ref, what=""):
    """got = (p, m, v) fp32; ref = ref64(...).  Prints the worst ratios before asserting."""
    p2, m1, v1, (bp, bm, bv) = ref
    tiny = 1e-300
    rp = ((got[0].double() - p2).abs() / (bp + tiny)).max().item()
    rm = ((got[1].double() - m1).abs() / (bm + tiny)).max().item()
    rv = ((got[2].double() - v1).abs() / (bv + tiny)).max().item()
    print(f"adamw bound ratios {what}: p {rp:.3f} m {rm:.3f} v {rv:.3f}")
    assert (got[0].double() - p2).abs().le(bp).all(), f"p outside the bound {what}: ratio {rp}"
    assert (got[1].double() - m1).abs().le(bm).all(), f"m outside the bound {what}: ratio {rm}"
    assert (got[2].double() - v1).abs().le(bv).all(), f"v outside the bound {what}: ratio {rv}"


def replay32(p, g, m, v, s, variant="ok"):
    """Unfused fp32 replay of the sequence with torch ops (one rounding per op); ``variant``
    selects one of the wrong sequences the bound must reject."""
    m1 = m + s["w1"] * (g - m)
    v1 = s["b2"] * v + (s["w2"] * g) * g
    step = s["step_size"]
    if variant == "ok":
        den = v1.sqrt() / s["bc2_sqrt"] + s["eps"]
    elif variant == "eps_inside":
        den = (v1.sqrt() + s["eps"]) / s["bc2_sqrt"]
    elif variant == "no_bc2":
        den = v1.sqrt() + s["eps"]
    elif variant == "no_bc1":
        den = v1.sqrt() / s["bc2_sqrt"] + s["eps"]
        step = _f32(LR)
    return p * s["decay"] - step * (m1 / den), m1, v1


# ------------------------------------------------------------------ the bound itself
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 20000])
def test_unfused_fp32_replay_is_inside_the_bound(t):
    p, g, m, v = make_inputs(seed=t, zero_state=(t == 1))
    s = scalars32(t)
    check_bounds(replay32(p, g, m, v, s), ref64(p, g, m, v, s), f"replay t={t}")


@pytest.mark.parametrize("t", [1, 2, 10])
@pytest.mark.parametrize("variant", ["eps_inside", "no_bc2", "no_bc1"])
def test_wrong_sequences_leave_the_bound(t, variant):
    p, g, m, v = make_inputs(seed=t, zero_state=(t == 1))
    s = scalars32(t)
    p2, _, _, (bp, _, _) = ref64(p, g, m, v, s)
    got = replay32(p, g, m, v, s, variant)[0]
    frac = ((got.double() - p2).abs() > bp).double().mean().item()
    print(f"adamw mutant {variant} t={t}: {100 * frac:.1f} % of the elements outside the p bound")
    assert frac > 0.4


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 20000])
def test_cpu_path_is_inside_the_bound(t):
    p, g, m, v = make_inputs(seed=100 + t, zero_state=(t == 1))
    model = Vec(N, p)
    opt = FusedAdamW(model, lr=LR, weight_decay=WD)
    fs = opt.flat
    opt.exp_avg, opt.exp_avg_sq = torch.zeros_like(fs.params), torch.zeros_like(fs.params)
    fs.view(opt.exp_avg, "w").copy_(m)
    fs.view(opt.exp_avg_sq, "w").copy_(v)
    opt.set_state_counter(t - 1)
    fs.reattach_grads()
    fs.view(fs.grads, "w").copy_(g)
    opt.step()
    assert opt.schedule_step() == t
    got = (model.w.detach(), fs.view(opt.exp_avg, "w"), fs.view(opt.exp_avg_sq, "w"))
    check_bounds(got, ref64(p, g, m, v, scalars32(t)), f"cpu path t={t}")


# ------------------------------------------------------------------ against torch.optim.AdamW
def test_each_of_five_steps_matches_torch_under_the_bound():
    """For k = 1..5: torch's state after k - 1 steps is loaded into a FusedAdamW, both take
    step k with the same gradient, and ours is compared with torch's per element.  (Five
    free-running steps are not compared: the drift compounds.)"""
    p0 = make_inputs(seed=1)[0]
    tp = torch.nn.Parameter(p0.clone())
    topt = torch.optim.AdamW([tp], lr=LR, weight_decay=WD)
    for k in range(1, 6):
        g = make_inputs(seed=10 + k)[1]
        model = Vec(N, tp.detach())
        opt = FusedAdamW(model, lr=LR, weight_decay=WD)
        opt.load_state_dict(topt.state_dict())
        assert opt.schedule_step() == k - 1
        if k == 1:
            m_prev, v_prev = torch.zeros(N), torch.zeros(N)
        else:
            m_prev, v_prev = topt.state[tp]["exp_avg"].clone(), topt.state[tp]["exp_avg_sq"].clone()
        p_prev = tp.detach().clone()
        opt.flat.reattach_grads()
        model.w.grad.copy_(g)
        tp.grad = g.clone()
        opt.step()
        topt.step()
        ref = ref64(p_prev, g, m_prev, v_prev, scalars32(k))
        st = topt.state[tp]
        check_bounds((tp.detach(), st["exp_avg"], st["exp_avg_sq"]), ref, f"torch step {k}")
        sd = opt.state_dict()["state"][0]
        check_bounds((model.w.detach(), sd["exp_avg"], sd["exp_avg_sq"]), ref, f"ours step {k}")
        # the two differ from each other by at most the two bounds
        assert (model.w.detach().double() - tp.detach().double()).abs().le(2 * ref[3][0]).all()
        assert float(sd["step"]) == float(st["step"]) == k


def _simplecnn_pair():
    from ddp_amd.models import SimpleCNN, reference_simple_cnn

    torch.manual_seed(0)
    ours, ref = SimpleCNN(), reference_simple_cnn()
    ref.load_state_dict(ours.state_dict())
    return ours, ref


def test_state_dict_has_torch_adamw_format_and_loads_both_ways():
    ours, ref = _simplecnn_pair()
    opt = FusedAdamW(ours, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05)
    topt = torch.optim.AdamW(ref.parameters(), lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05)
    a, b = opt.state_dict(), topt.state_dict()
    assert a["state"] == {} and b["state"] == {}
    assert list(a["param_groups"][0]) == list(b["param_groups"][0])
    assert a["param_groups"] == b["param_groups"]
    x, y = torch.rand(4, 1, 28, 28), torch.randint(0, 10, (4,))
    for m, o in ((ours, opt), (ref, topt)):
        o.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        o.step()
    a, b = opt.state_dict(), topt.state_dict()
    assert list(a) == list(b) and list(a["param_groups"][0]) == list(b["param_groups"][0])
    assert a["param_groups"] == b["param_groups"]
    assert list(a["state"]) == list(b["state"])
    for i in b["state"]:
        assert list(a["state"][i]) == list(b["state"][i]) == ["step", "exp_avg", "exp_avg_sq"]
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert a["state"][i][k].shape == b["state"][i][k].shape and a["state"][i][k].dtype == b["state"][i][k].dtype
        assert float(a["state"][i]["step"]) == 1.0
        assert torch.allclose(a["state"][i]["exp_avg"], b["state"][i]["exp_avg"], rtol=1e-4, atol=1e-7)
    # torch loads ours
    ref2 = _simplecnn_pair()[1]
    t2 = torch.optim.AdamW(ref2.parameters())
    t2.load_state_dict(a)
    assert t2.param_groups[0]["betas"] == (0.8, 0.99)
    assert torch.equal(t2.state[next(iter(ref2.parameters()))]["exp_avg"], a["state"][0]["exp_avg"])
    # ours loads torch's
    ours2 = _simplecnn_pair()[0]
    o2 = FusedAdamW(ours2)
    o2.load_state_dict(b)
    assert o2.schedule_step() == 1 and o2.steps == 1
    assert o2.param_groups[0]["betas"] == (0.8, 0.99) and o2.param_groups[0]["lr"] == 2e-3
    c = o2.state_dict()
    for i in b["state"]:
        assert torch.equal(c["state"][i]["exp_avg_sq"], b["state"][i]["exp_avg_sq"])
    bad = topt.state_dict()
    bad["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        o2.load_state_dict(bad)


def test_schedule_shares_the_counter_and_load_keeps_the_base_rate():
    sched = LRSchedule(1e-2, 6, "cosine", warmup_steps=2)
    model = Vec(100, torch.ones(100))
    opt = FusedAdamW(model, lr=1e-2, lr_schedule=sched)
    assert opt.schedule_step() == 0 and opt.current_lr() == sched.lr_at(0)
    for k in range(3):
        opt.flat.reattach_grads()
        model.w.grad.fill_(0.5)
        opt.step()
    assert opt.schedule_step() == 3 and opt.current_lr() == sched.lr_at(3)
    sd = opt.state_dict()
    assert sd["param_groups"][0]["lr"] == sched.lr_at(3)  # the next step's rate
    assert float(sd["state"][0]["step"]) == 3.0
    fresh = FusedAdamW(Vec(100), lr=1e-2, lr_schedule=sched)
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]["lr"] == 1e-2 and fresh.loaded_lr == sched.lr_at(3)
    assert fresh.schedule_step() == 3 and fresh.current_lr() == sched.lr_at(3)
    plain = FusedAdamW(Vec(100))
    assert plain.schedule_step() == 0  # there without a schedule: it is the Adam step


# ------------------------------------------------------------------ coefficient table
def test_coef_table_entries_length_and_saturation():
    tab = coef_table(LR, (B1, B2), WD)
    assert tab.dtype == torch.float32 and tab.dim() == 2 and tab.shape[1] == 4
    n = tab.shape[0]
    for t in (0, 1, 9, 999, n - 2, n - 1):
        want = torch.tensor(coef_entry(t, LR, B1, B2, WD), dtype=torch.float64).to(torch.float32)
        assert torch.equal(tab[t], want), t
    k = 10
    assert tab[k - 1, 1].item() == _f32(LR / (1 - B1 ** k)) and tab[k - 1, 2].item() == _f32((1 - B2 ** k) ** 0.5)
    assert tab[k - 1, 0].item() == _f32(1 - LR * WD) and tab[k - 1, 3].item() == _f32(LR)

    # the length rule: the last entry is the first whose corrections have both rounded away ...
    def saturated(t):
        e = coef_entry(t, LR, B1, B2, WD)
        return _f32(e[1]) == _f32(LR) and _f32(e[2]) == 1.0

    assert saturated(n - 1) and not saturated(n - 2)
    # ... so it holds past the end: the closed form of any later step rounds to the same entry
    for t in (n, n + 1, 10 * n, (1 << 20) - 1):
        want = torch.tensor(coef_entry(t, LR, B1, B2, WD), dtype=torch.float64).to(torch.float32)
        assert torch.equal(want, tab[n - 1]), t


def test_coef_table_with_a_schedule():
    sched = LRSchedule(3e-3, 40, "cosine", warmup_steps=5)
    tab = coef_table(3e-3, (B1, B2), WD, sched)
    assert torch.equal(tab[:40, 3], sched.table)
    assert (tab[40:, 3] == sched.table[-1]).all()  # past the schedule its last rate holds
    assert tab.shape[0] == coef_table(sched.lr_at(39), (B1, B2), WD).shape[0]
    for t in (0, 7, 39, 41):
        lr_t = sched.lr_at(t)
        want = torch.tensor(coef_entry(t, lr_t, B1, B2, WD), dtype=torch.float64).to(torch.float32)
        assert torch.equal(tab[t], want), t
    # betas that saturate at once: the schedule's length wins
    short = coef_table(3e-3, (0.0, 0.0), WD, sched)
    assert short.shape[0] == 40 and coef_table(3e-3, (0.0, 0.0), WD).shape[0] == 1


def test_coef_table_refuses_betas_that_do_not_saturate():
    with pytest.raises(ValueError, match="do not round to 1"):
        coef_table(LR, (0.9, 0.99999), WD)
    with pytest.raises(ValueError):
        FusedAdamW(Vec(8), betas=(0.9, 0.99999)).coef_table()


# ------------------------------------------------------------------ two ranks over gloo
def _worker_adamw(rank, ws, port, ckdir, epochs, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import TrainOptions, ddp_train, replica_digest
    import ddp_amd.engine.trainer as tr

    seen = {}
    orig_verify = tr.verify_replicas

    def verify(fs, opt, rank_, ws_, epoch):
        seen.setdefault("start_step", opt.schedule_step() - 4)  # 4 steps into this run's first epoch
        seen["step"] = opt.schedule_step()
        seen["digest"] = replica_digest(fs, opt)
        return orig_verify(fs, opt, rank_, ws_, epoch)

    tr.verify_replicas = verify
    opts = TrainOptions(backend="gloo", checkpoint_dir=ckdir, max_steps=4, num_workers=0, log_every=1000,
                        data="synthetic", optimizer="adamw", lr=1e-3, weight_decay=1e-2, verify_replicas=True)
    ddp_train(rank, ws, epochs, 16, opts)
    q.put((rank, seen["start_step"], seen["step"], seen["digest"]))


@pytest.mark.slow
def test_two_ranks_adamw_verify_replicas_and_resume(tmp_path, capfd):
    """--optimizer adamw --verify_replicas over gloo: replicas stay bitwise equal (a divergence
    raises in the workers), and a third epoch started from the checkpoints resumes on BOTH
    ranks at optimizer step 8 - rank 1 gets the counter and both moments by broadcast."""
    from ddp_amd.parallel import free_port

    ck = str(tmp_path / "checkpoints")
    q = mp.get_context("spawn").Queue()
    mp.start_processes(_worker_adamw, args=(2, free_port(), ck, 2, q), nprocs=2, start_method="spawn", join=True)
    res = sorted(q.get() for _ in range(2))
    assert [r[1] for r in res] == [0, 0] and [r[2] for r in res] == [8, 8]
    assert res[0][3] == res[1][3]
    assert sorted(os.listdir(ck)) == ["epoch_0.pt", "epoch_1.pt"]
    sd = torch.load(os.path.join(ck, "epoch_1.pt"), weights_only=True)["optimizer"]
    assert float(sd["state"][0]["step"]) == 8.0
    out = capfd.readouterr().out
    assert "replicas bitwise identical after epoch 1" in out
    mp.start_processes(_worker_adamw, args=(2, free_port(), ck, 3, q), nprocs=2, start_method="spawn", join=True)
    res = sorted(q.get() for _ in range(2))
    assert [r[1] for r in res] == [8, 8], "both ranks resume at step 8"
    assert [r[2] for r in res] == [12, 12]
    assert res[0][3] == res[1][3]
    out = capfd.readouterr().out
    assert "Starting epoch 0" not in out and "Rank 1: Starting epoch 2" in out
    assert "replicas bitwise identical after epoch 2" in out
    assert "WARNING" not in out


# ------------------------------------------------------------------ options
def test_option_errors():
    import train_ddp
    from ddp_amd.engine.trainer import TrainOptions, check_fused_engine_options, validate_options

    with pytest.raises(ValueError, match="--momentum"):
        validate_options(TrainOptions(optimizer="adamw", momentum=0.9))
    with pytest.raises(ValueError, match="--optimizer adamw needs the module path"):
        validate_options(TrainOptions(optimizer="adamw", device="gpu"))
    with pytest.raises(ValueError, match="--optimizer adamw"):
        check_fused_engine_options(TrainOptions(optimizer="adamw"), True)
    validate_options(TrainOptions(optimizer="adamw", device="gpu", engine="module"))
    validate_options(TrainOptions(optimizer="adamw", device="gpu", model="resnet18"))
    with pytest.raises(ValueError, match="--optimizer"):
        validate_options(TrainOptions(optimizer="lamb"))
    a = train_ddp.parse_args(["--optimizer", "adamw", "--beta1", "0.8", "--beta2", "0.95", "--adam_eps", "1e-6"])
    assert (a.optimizer, a.beta1, a.beta2, a.adam_eps) == ("adamw", 0.8, 0.95, 1e-6)
    assert train_ddp.parse_args([]).optimizer == "sgd"
    with pytest.raises(ValueError, match="--momentum"):
        train_ddp.main(["--optimizer", "adamw", "--momentum", "0.9", "--device", "cpu"])
