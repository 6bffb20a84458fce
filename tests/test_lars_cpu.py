"""FusedLARS on the CPU: the rule, its a-priori bounds, three wrong variants that must miss them,
the state dict, the schedule, two ranks over gloo, option errors.

The bounds (ddp_amd/ops/kernel_bounds.py ``trust_ratio_bound`` and ``lars_reference``, whose
docstrings carry the same derivation next to the code) follow from the operation order in the
header of csrc/kernels/lars.hip, with u = 2^-24:

* ratio.  A tensor's sum of squares S has non-negative terms, each behind a chain of at most
  k = 1 + 2 + 2 + 6 + 3 + ceil(items / 64) + 6 roundings (square; the thread's folds; the wave
  tree; the block's four waves; the lane's sequential sum over item partials; the last wave
  tree), so |S - s| <= gamma_k s with gamma_k = k u / (1 - k u).  The correctly rounded root
  halves that and adds one rounding: e_n = (gamma_k / 2 + u)(1 + gamma_k) for wn and for gn -
  half the chain length of each norm's summation.  Then the handful of roundings of the ratio
  itself: trust_coef * wn (u); with clipping gn * coef (u); fma(wd, wn, gn) and + eps (2 u:
  all terms are non-negative, relative errors do not grow); the division (u).  To first order
  rho = 2 e_n + 5 u (6 u with clipping), times 1 + 2^-10 for the second-order terms.
* p and m, per element, magnitudes as sums of absolute values, every decay / momentum
  multiply-add counted as two roundings (the kernel's fma has one; the torch path's separate
  multiply and add have two):
      d0 = coef g                e0 = u |d0|                  (0 without clipping)
      d1 = wd w + d0             e1 = e0 + 2 u A1,  A1 = |wd w| + |d0|   (e0 without decay)
      d2 = R d1                  e2 = R e1 + (rho + u) A2,  A2 = R A1
      buf = d2 (first step)      eb = e2, Ab = A2
      buf = (1 - damp) d2 + mom m   eb = (1 - damp) e2 + 3 u (1 - damp) A2 + 2 u |mom m|
      d3 = d2 + mom buf (nesterov; else buf)   e3 = e2 + mom eb + 2 u A3,  A3 = A2 + mom Ab
      p' = w - lr d3             ep = lr e3 + u lr A3 + u (|w| + lr A3)
  eb bounds the momentum buffer, ep the parameter, both times 1 + 2^-10.
Nothing here is fitted to an output: every test prints the worst |error| / bound it saw."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from ddp_amd.ops import FusedLARS, FusedSGD, LRSchedule
from ddp_amd.ops import kernel_bounds as kb
from ddp_amd.ops.lars import ITEM, lars_layout

# tensor lengths of the synthetic layout: 1, 3, 4, 5, 63, 64, 65, one item, one item + 1, three items + 7
LENS = [1, 3, 4, 5, 63, 64, 65, ITEM, ITEM + 1, 3 * ITEM + 7]
EXCLUDED = {1, 3}          # (lengths 3 and 5): ratio 1, no decay
ZERO_W, ZERO_G = 4, 6      # all-zero weights / all-zero gradient
BEGINS = [int(b) for b in np.cumsum([0] + [-(-m // 64) * 64 for m in LENS[:-1]])]
N = BEGINS[-1] + -(-LENS[-1] // 64) * 64
SEGS = list(zip(BEGINS, LENS))
WD, TC, EPS, LR, MOM = 0.1, 0.02, 1e-8, 0.05, 0.9
WDS = [0.0 if i in EXCLUDED else WD for i in range(len(LENS))]
ADAPTS = [i not in EXCLUDED for i in range(len(LENS))]
COEF = 0.37


def make_inputs(seed=0):
    """Flat float32 (w, g, m) with zero padding; weight scales 0.1 / 1 / 10 and gradient scales
    1 .. 1e-3 by tensor, so per-tensor and whole-buffer norms differ by orders of magnitude."""
    gen = torch.Generator().manual_seed(seed)
    w, g, m = torch.zeros(N), torch.zeros(N), torch.zeros(N)
    for i, (b, n) in enumerate(SEGS):
        w[b:b + n] = torch.randn(n, generator=gen) * 10.0 ** (i % 3 - 1)
        g[b:b + n] = torch.randn(n, generator=gen) * 10.0 ** -(i % 4)
        m[b:b + n] = torch.randn(n, generator=gen) * 10.0 ** -(i % 4) * 0.05
    w[BEGINS[ZERO_W]:BEGINS[ZERO_W] + LENS[ZERO_W]] = 0
    g[BEGINS[ZERO_G]:BEGINS[ZERO_G] + LENS[ZERO_G]] = 0
    return w, g, m


def reference(w, g, m, momentum=MOM, nesterov=False, maximize=False, first=False, coef=None, dampening=0.0,
              wds=WDS, adapts=ADAPTS, lr=LR):
    return kb.lars_reference(w.numpy(), g.numpy(), None if m is None else m.numpy(), SEGS, wds, adapts, lr, momentum,
                             dampening, nesterov, maximize, first, TC, EPS, coef)


def check_bounds(p, m, ref, what, ratios=None):
    """Every element of p (and m, when given) inside its bound; prints the worst |err| / bound."""
    p64, m64, r64, bp, bm = ref
    worst = {}
    for name, got, want, bound in (("p", p, p64, bp), ("m", m, m64, bm)):
        if got is None:
            continue
        err = np.abs(got.double().numpy() - want)
        assert np.isfinite(err).all(), f"{what}: non-finite {name}"
        bad = err > bound
        worst[name] = float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
        assert not bad.any(), f"{what}: {int(bad.sum())} elements of {name} outside the bound, first at {int(np.argmax(bad))}"
    if ratios is not None:
        rel = [abs(float(r) - R) / R / max(kb.trust_ratio_bound(n, False), 1e-300)
               for r, R, n, a in zip(ratios, r64, LENS, ADAPTS) if a and R != 1.0]
        worst["ratio"] = max(rel)
        for i, (r, R) in enumerate(zip(ratios, r64)):
            lim = kb.trust_ratio_bound(LENS[i], True) * R if ADAPTS[i] and R != 1.0 else 0.0
            assert abs(float(r) - R) <= lim, f"{what}: ratio of tensor {i}: {float(r)!r} vs {R!r}"
    print(f"[lars bound] {what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


class Bag(torch.nn.Module):
    """Parameters t00 .. t09 of the lengths LENS, registered in reverse so that the flat order
    (reverse registration) is ascending: the flat layout is BEGINS."""

    def __init__(self, w=None, shapes=None):
        super().__init__()
        for i in reversed(range(len(LENS))):
            shape = (LENS[i],) if shapes is None else shapes[i]
            v = torch.zeros(shape) if w is None else w[BEGINS[i]:BEGINS[i] + LENS[i]].clone().view(shape)
            setattr(self, f"t{i:02d}", torch.nn.Parameter(v))


def by_index(name, shape):
    return int(name[1:]) in EXCLUDED


def bag_opt(w, g, **kw):
    model = Bag(w)
    kw.setdefault("exclude", by_index)
    opt = FusedLARS(model, lr=LR, weight_decay=WD, trust_coef=TC, eps=EPS, **kw)
    fs = opt.flat
    assert [fs.offsets[n] for n in fs.names] == BEGINS and fs.numel == N
    fs.grads.copy_(g)
    return opt


# ------------------------------------------------------------------------------- layout
def test_layout_is_a_function_of_the_shapes():
    segs, items, cmap = lars_layout(BEGINS, LENS, N, WDS, ADAPTS)
    assert segs.shape == (10, 8) and cmap.shape == (N // 64,) and items.shape == (sum(-(-m // ITEM) for m in LENS), 4)
    assert segs[:, 3].tolist() == [1] * 8 + [2, 4] and segs[:, 2].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
    assert items[-4:, 1].tolist() == [ITEM, ITEM, ITEM, 7] and items[-4:, 3].tolist() == [0, 1, 2, 3]
    assert items[8:10, 1].tolist() == [ITEM, 1]
    assert bool((items[:, 1] <= ITEM).all())
    assert cmap[BEGINS[4] // 64].item() == 4 and cmap[BEGINS[6] // 64 + 1].item() == 6
    assert cmap[BEGINS[9] // 64 + (3 * ITEM) // 64].item() == 9
    # padding-only chunks (none in this layout: every chunk holds part of a tensor) map to the null segment
    s2, i2, c2 = lars_layout([0, 128], [1, 1], 256, [0, 0], [1, 1])
    assert c2.tolist() == [0, 2, 1, 2]
    again = lars_layout(BEGINS, LENS, N, WDS, ADAPTS)
    assert all(torch.equal(a, b) for a, b in zip((segs, items, cmap), again))
    with pytest.raises(ValueError):
        lars_layout([0, 32], [1, 1], 128, [0, 0], [1, 1])


def test_replayed_norm_is_inside_its_chain_bound():
    w, g, _ = make_inputs(3)
    for i, (b, n) in enumerate(SEGS):
        x = g[b:b + n].numpy()
        s32, s64 = kb.replay_seg_sqnorm(x), float((x.astype(np.float64) ** 2).sum())
        k = kb.seg_sqnorm_chain(n)
        assert abs(float(s32) - s64) <= k * kb.U / (1 - k * kb.U) * s64, i
    assert kb.seg_sqnorm_chain(3 * ITEM + 7) == 21 and kb.seg_sqnorm_chain(65 * ITEM) == 22


# ------------------------------------------------------------------------------- the bound
CASES = {  # momentum, nesterov, maximize, clip
    "plain": (0.0, False, False, False), "momentum": (MOM, False, False, False),
    "nesterov": (MOM, True, False, False), "maximize": (MOM, False, True, False), "clip": (MOM, False, False, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cpu_path_and_rounded_reference_meet_the_bounds(case):
    """Two CPU steps (the momentum-initialising first one and a regular one) against the float64
    rule; the float64 rule rounded to float32 is inside the same bounds."""
    mom, nesterov, maximize, clip = CASES[case]
    w, g, _ = make_inputs(1)
    _, g2, _ = make_inputs(2)
    max_norm = COEF * float(g.double().norm()) if clip else None  # (the first step clips with about COEF)
    opt = bag_opt(w, g, momentum=mom, nesterov=nesterov, maximize=maximize, max_grad_norm=max_norm)
    p, mbuf = w, None
    for step, grad in enumerate((g, g2)):
        opt.flat.grads.copy_(grad)
        opt.step()
        coef = opt.grad_clip_stats()["coef"] if clip else None
        ref = reference(p, grad, mbuf, momentum=mom, nesterov=nesterov, maximize=maximize, first=step == 0, coef=coef)
        st = opt.trust_stats()
        ratios = [st[f"t{i:02d}"]["ratio"] for i in range(len(LENS))]
        check_bounds(opt.flat.params, opt.momentum_buffer, ref, f"cpu {case} step {step}", ratios)
        check_bounds(torch.from_numpy(ref[0]).float(), torch.from_numpy(ref[1]).float() if mom else None, ref,
                     f"rounded float64 {case} step {step}")
        if step == 0:
            assert st["t04"]["ratio"] == 1.0 and not st["t01"]["adapted"] and st["t02"]["adapted"]
        p, mbuf = opt.flat.params.clone(), None if opt.momentum_buffer is None else opt.momentum_buffer.clone()


def rule64(w, g, m, variant=None):
    """The rule written out per tensor in float64 (momentum MOM, a regular step), or one of
    three wrong variants: "decay_after" (decay added after the ratio), "no_wd_term" (the ratio
    without wd * wn), "global" (one ratio from whole-buffer norms)."""
    w, g, m = (x.double() for x in (w, g, m))
    p = w.clone()
    WN, GN = w.norm(), g.norm()
    for i, (b, n) in enumerate(SEGS):
        ww, gg, mm = w[b:b + n], g[b:b + n], m[b:b + n]
        wd = WDS[i]
        wn, gn = (WN, GN) if variant == "global" else (ww.norm(), gg.norm())
        den = gn + EPS if variant == "no_wd_term" else wd * wn + gn + EPS
        R = float(np.float32(TC)) * wn / den if ADAPTS[i] and wn > 0 and gn > 0 else 1.0
        wd32, mom32, lr32 = float(np.float32(wd)), float(np.float32(MOM)), float(np.float32(LR))
        d = gg * R + wd32 * ww if variant == "decay_after" else (gg + wd32 * ww) * R
        p[b:b + n] = ww - lr32 * (mom32 * mm + d)
    return p


def test_three_wrong_variants_miss_the_bound():
    w, g, m = make_inputs(1)
    p64, _, _, bp, _ = reference(w, g, m)
    adapted = np.zeros(N, dtype=bool)
    for i, (b, n) in enumerate(SEGS):
        adapted[b:b + n] = ADAPTS[i]
    good = np.abs(rule64(w, g, m).numpy() - p64)
    assert (good <= bp).all(), "the independent float64 rule must agree with the reference"
    for variant in ("decay_after", "no_wd_term", "global"):
        err = np.abs(rule64(w, g, m, variant).numpy() - p64)
        out = (err > bp) & adapted
        assert out.any(), variant
        print(f"[lars mutant] {variant}: {int(out.sum())} adapted elements outside, worst error / bound "
              f"{float((err[out] / bp[out]).max()):.3g}")


# ------------------------------------------------------------------------------- rule cases
def test_rule_cases():
    w, g, _ = make_inputs(1)
    opt = bag_opt(w, g, momentum=0.0)
    opt.step()
    st = opt.trust_stats()
    assert st["t04"]["w_norm"] == 0.0 and st["t04"]["ratio"] == 1.0      # zero weights
    assert st["t06"]["g_norm"] == 0.0 and st["t06"]["ratio"] == 1.0      # zero gradient
    assert st["t07"]["ratio"] not in (0.0, 1.0) and st["t07"]["adapted"]
    close = dict(rtol=4 * kb.U, atol=1e-9)  # (a few roundings: torch may or may not fuse p + alpha * d)
    for i in EXCLUDED:  # excluded: plain SGD, no decay
        b, n = SEGS[i]
        assert torch.allclose(opt.flat.params[b:b + n], w[b:b + n] - LR * g[b:b + n], **close)
        assert st[f"t{i:02d}"]["ratio"] == 1.0 and not st[f"t{i:02d}"]["adapted"]
    b, n = SEGS[ZERO_G]  # zero gradient, adapted: ratio 1 and the decay alone
    assert torch.allclose(opt.flat.params[b:b + n], w[b:b + n] - LR * (WD * w[b:b + n]), **close)
    # exclude="1d" (the default) excludes every 1-D parameter of this model; None excludes none
    o1 = bag_opt(w, g, momentum=0.0, exclude="1d")
    assert all(o1.excluded(n) for n in o1.flat.names)
    o1.step()
    assert torch.allclose(o1.flat.params, w - LR * g, **close)
    o2 = bag_opt(w, g, momentum=0.0, exclude=None)
    assert not any(o2.excluded(n) for n in o2.flat.names)
    o2.step()
    assert all(v["adapted"] for v in o2.trust_stats().values()) and o2.trust_stats()["t01"]["ratio"] != 1.0
    # a matrix is adapted under "1d"
    shapes = [(m,) for m in LENS]
    shapes[5] = (8, 8)
    o3 = FusedLARS(Bag(w, shapes), lr=LR)
    assert [n for n in o3.flat.names if not o3.excluded(n)] == ["t05"]
    seen = []
    o4 = FusedLARS(Bag(w, shapes), lr=LR, exclude=lambda name, shape: seen.append((name, shape)) or name == "t05")
    assert [n for n in o4.flat.names if o4.excluded(n)] == ["t05"] and ("t05", (8, 8)) in seen
    for bad in (dict(trust_coef=0.0), dict(eps=-1.0), dict(exclude="2d"), dict(nesterov=True, momentum=0.0),
                dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            FusedLARS(Bag(w), lr=LR, **bad)


# ------------------------------------------------------------------------------- state dict
def test_state_dict_is_sgds_and_loads_both_ways():
    from ddp_amd.models import SimpleCNN, reference_simple_cnn

    torch.manual_seed(0)
    model = SimpleCNN()
    opt = FusedLARS(model, lr=0.02, momentum=0.9, weight_decay=1e-4, trust_coef=0.01)
    assert opt.state_dict()["state"] == {}
    for q in model.parameters():
        q.grad.normal_()
    opt.step()
    sd = opt.state_dict()
    ref = reference_simple_cnn()
    topt = torch.optim.SGD(ref.parameters(), lr=0.5)
    tkeys = [k for k in topt.state_dict()["param_groups"][0] if k != "params"]
    assert list(sd["param_groups"][0]) == [*tkeys, "trust_coef", "eps", "exclude", "params"]
    assert sd["param_groups"][0]["exclude"] == "1d" and sd["param_groups"][0]["trust_coef"] == 0.01
    for i, q in enumerate(ref.parameters()):
        assert set(sd["state"][i]) == {"momentum_buffer"} and sd["state"][i]["momentum_buffer"].shape == q.shape
    topt.load_state_dict(sd)  # torch.optim.SGD loads a LARS checkpoint
    assert topt.param_groups[0]["lr"] == 0.02 and topt.param_groups[0]["momentum"] == 0.9
    assert all(torch.equal(topt.state[q]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
               for i, q in enumerate(ref.parameters()))
    fsgd = FusedSGD(SimpleCNN(), lr=0.5)
    fsgd.load_state_dict(sd)  # and so does FusedSGD
    assert fsgd.param_groups[0]["momentum"] == 0.9 and torch.equal(fsgd.momentum_buffer, opt.momentum_buffer)
    tsd = topt.state_dict()  # (torch carries a loaded group's extra keys along: a plain SGD checkpoint has none)
    tsd["param_groups"] = [{k: v for k, v in tsd["param_groups"][0].items() if k in (*tkeys, "params")}]
    for src in (tsd, fsgd.state_dict()):  # and back: missing keys keep the constructor's values
        o2 = FusedLARS(SimpleCNN(), lr=0.5, trust_coef=0.03, exclude=None)
        o2.load_state_dict(src)
        g2 = o2.param_groups[0]
        assert (g2["lr"], g2["momentum"], g2["weight_decay"], g2["trust_coef"], g2["exclude"]) == (0.02, 0.9, 1e-4, 0.03, None)
        assert torch.equal(o2.momentum_buffer, opt.momentum_buffer) and o2.steps >= 1
    o3 = FusedLARS(SimpleCNN(), lr=0.5, exclude=None)
    o3.load_state_dict(sd)
    assert o3.param_groups[0]["exclude"] == "1d" and o3.param_groups[0]["trust_coef"] == 0.01
    o4 = FusedLARS(SimpleCNN(), lr=0.5, exclude=lambda n, s: False)
    assert o4.state_dict()["param_groups"][0]["exclude"] == "callable"
    with pytest.raises(ValueError):
        FusedLARS(Bag(), lr=0.1).load_state_dict(sd)


# ------------------------------------------------------------------------------- schedule
def test_ratios_compose_with_the_schedule_and_resume_in_sequence():
    rates = [0.05, 0.02, 0.08, 0.01]
    w, _, _ = make_inputs(1)
    grads = [make_inputs(10 + k)[1] for k in range(4)]
    sched = bag_opt(w, grads[0], lr_schedule=LRSchedule.from_values(rates))
    byval = bag_opt(w, grads[0])
    saved = None
    for k, g in enumerate(grads):
        if k == 2:
            saved = (sched.flat.params.clone(), sched.state_dict())
        for o in (sched, byval):
            o.flat.grads.copy_(g)
        assert sched.current_lr() == float(np.float32(rates[k]))
        byval.param_groups[0]["lr"] = float(np.float32(rates[k]))
        sched.step()
        byval.step()
        assert torch.equal(sched.flat.params, byval.flat.params), k
        assert sched.trust_stats() == byval.trust_stats()
    assert sched.schedule_step() == 4
    resumed = bag_opt(saved[0], grads[2], lr_schedule=LRSchedule.from_values(rates))
    resumed.load_state_dict(saved[1])
    resumed.set_schedule_step(2)
    for g in grads[2:]:
        resumed.flat.grads.copy_(g)
        resumed.step()
    assert torch.equal(resumed.flat.params, sched.flat.params)
    assert torch.equal(resumed.momentum_buffer, sched.momentum_buffer)


# ------------------------------------------------------------------ two ranks over gloo
def _worker_lars(rank, ws, port, ckdir, epochs, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import TrainOptions, ddp_train, replica_digest
    import ddp_amd.engine.trainer as tr

    seen = {}
    orig_verify = tr.verify_replicas

    def verify(fs, opt, rank_, ws_, epoch):
        seen["digest"] = replica_digest(fs, opt)
        seen["ratios"] = sorted(v["ratio"] for v in opt.trust_stats().values())
        return orig_verify(fs, opt, rank_, ws_, epoch)

    tr.verify_replicas = verify
    opts = TrainOptions(backend="gloo", checkpoint_dir=ckdir, max_steps=4, num_workers=0, log_every=1000,
                        data="synthetic", optimizer="lars", lr=0.5, momentum=0.9, weight_decay=1e-3,
                        trust_coef=0.02, verify_replicas=True)
    ddp_train(rank, ws, epochs, 16, opts)
    q.put((rank, seen["digest"], seen["ratios"]))


@pytest.mark.slow
def test_two_ranks_lars_verify_replicas_and_resume(tmp_path, capfd):
    """--optimizer lars --verify_replicas over gloo: replicas stay bitwise equal over two epochs
    (a divergence raises in the workers; both ranks hold the same ratios), and a third epoch
    started from the checkpoints ends bitwise where an uninterrupted three-epoch run ends."""
    from ddp_amd.parallel import free_port

    def run(ck, epochs):
        q = mp.get_context("spawn").Queue()
        mp.start_processes(_worker_lars, args=(2, free_port(), ck, epochs, q), nprocs=2, start_method="spawn", join=True)
        res = sorted(q.get() for _ in range(2))
        assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
        assert any(r != 1.0 for r in res[0][2])
        return res

    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    run(a, 2)
    assert "replicas bitwise identical after epoch 1" in capfd.readouterr().out
    assert sorted(os.listdir(a)) == ["epoch_0.pt", "epoch_1.pt"]
    resumed = run(a, 3)
    out = capfd.readouterr().out
    assert "Starting epoch 0" not in out and "Rank 1: Starting epoch 2" in out and "WARNING" not in out
    straight = run(b, 3)
    assert resumed[0][1] == straight[0][1], "the resumed run must end where the uninterrupted run ends"
    ca = torch.load(os.path.join(a, "epoch_2.pt"), weights_only=True)
    cb = torch.load(os.path.join(b, "epoch_2.pt"), weights_only=True)
    assert all(torch.equal(ca["model"][k], cb["model"][k]) for k in ca["model"])
    assert ca["optimizer"]["param_groups"] == cb["optimizer"]["param_groups"]
    assert ca["optimizer"]["param_groups"][0]["trust_coef"] == 0.02
    for i, s in ca["optimizer"]["state"].items():
        assert torch.equal(s["momentum_buffer"], cb["optimizer"]["state"][i]["momentum_buffer"])


# ------------------------------------------------------------------ options
def test_option_errors_and_parsing():
    import train_ddp
    from ddp_amd.engine.trainer import TrainOptions, check_fused_engine_options, validate_options
    import ddp_amd.ops as ops

    assert "FusedLARS" in ops.__all__
    with pytest.raises(ValueError, match="--optimizer lars needs the module path"):
        validate_options(TrainOptions(optimizer="lars", device="gpu"))
    with pytest.raises(ValueError, match="--optimizer lars"):
        check_fused_engine_options(TrainOptions(optimizer="lars"), True)
    validate_options(TrainOptions(optimizer="lars", momentum=0.9, device="gpu", engine="module"))
    validate_options(TrainOptions(optimizer="lars", device="gpu", model="resnet18"))
    with pytest.raises(ValueError, match="--trust_coef"):
        validate_options(TrainOptions(optimizer="lars", trust_coef=0.0))
    with pytest.raises(ValueError, match="--lars_exclude"):
        validate_options(TrainOptions(optimizer="lars", lars_exclude="2d"))
    with pytest.raises(ValueError, match="--optimizer"):
        validate_options(TrainOptions(optimizer="lamb"))
    with pytest.raises(ValueError, match="--optimizer adamw needs the module path"):
        validate_options(TrainOptions(optimizer="adamw", device="gpu"))
    a = train_ddp.parse_args(["--optimizer", "lars", "--trust_coef", "0.02", "--lars_eps", "1e-6",
                              "--lars_exclude", "none", "--momentum", "0.9"])
    assert (a.optimizer, a.trust_coef, a.lars_eps, a.lars_exclude, a.momentum) == ("lars", 0.02, 1e-6, "none", 0.9)
    d = train_ddp.parse_args([])
    assert (d.optimizer, d.trust_coef, d.lars_eps, d.lars_exclude) == ("sgd", 1e-3, 1e-8, "1d")
    with pytest.raises(SystemExit):
        train_ddp.parse_args(["--lars_exclude", "2d"])
