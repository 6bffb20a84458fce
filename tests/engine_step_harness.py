"""One checked step of the fused SimpleCNN engine, for both precisions
(tests/test_engine_step_elementwise_gpu.py binds it to ``BF16``,
tests/test_engine_step_fp32_elementwise_gpu.py to ``FP32``): build the engine, snapshot what the
step reads, poison what it should write, run one eager step and hold everything it materialised
to tests/engine_step_cases.py ``check_step``.  A helper module, not a test module; importing it
needs neither a GPU nor the native extension.

What differs between the two precisions is the ``Precision`` description: the buffers poisoned
and the entry shadows, the model's compute dtype and the fixed engine options, which stages a
chain stores, which buffers must keep their NaN past a ragged batch's last row, how the set of
reported stages is checked, and what the engine must have resolved (fp32 only).
"""
import dataclasses
import typing

import torch

import engine_step_cases as E

dev = "cuda"
NAMES = {"w1": "net.0.weight", "b1": "net.0.bias", "w2": "net.2.weight", "b2": "net.2.bias", "wfc": "fl.weight",
         "bfc": "fl.bias"}
LR = 0.01


@dataclasses.dataclass(frozen=True)
class Precision:
    prec: str                          # check_step's table: "bf16" | "fp32"
    tag: str                           # "" | "fp32": the report's chain prefix, the messages' first word
    poison: tuple                      # buffers of eng.t filled with NaN before the step
    shadows: tuple                     # the entry shadows handed to check_step
    compute_dtype: typing.Any          # SimpleCNN(compute_dtype=): None keeps the model's default
    options: dict                      # EngineOptions a test may override (bf16: the level-0 defaults) or not
    stored: typing.Callable            # (level, l3) -> the buffers the chain materialises
    past_B: typing.Callable            # (l3) -> {buffer: elements per image} that keep NaN past row B
    check_setup: typing.Callable       # (eng): what the engine must have resolved
    check_plan: typing.Callable        # (eng, B, plan): the counts the reference derives are the engine's
    check_stages: typing.Callable      # (res, stored, level, momentum, fuse_opt): the stages reported


def _bf16_stored(level, l3):
    stored = ["a1", "a2", "dz2", "w2slab", "w1slab", "loss_hist"]
    stored += ["dz1"] if level == 0 else []
    stored += ["fc_part"] if not l3 else []                  # level 3 hands the partials over as granules
    stored += ["dlogits", "loss_rows"] if (level == 0 or l3) else []  # level 1: fc_bwd's prologue keeps them in LDS
    return stored


def _bf16_stages(res, stored, level, mom, fuse_opt):
    want = {"shadows", "a2", "dz2", "loss_hist", "w2slab", "w1slab", "grad_w1", "grad_b1", "grad_w2", "grad_b2", "grad_bfc"}
    want |= {f"param_{p}" for p in E.PARAMS} | {s for s in stored if s not in ("loss_hist",)}
    assert want <= set(res), sorted(want - set(res))


BF16 = Precision(
    prec="bf16", tag="",
    poison=("a1", "a2", "dz1", "dz2", "fc_part", "dlogits", "loss_rows", "w2slab", "w1slab"),
    shadows=("w2_bf16", "w2t_bf16", "wfc_frag", "wfc_bf16"),
    compute_dtype=None, options=dict(fuse_level=0, fuse_opt=True, store_a1=1),
    stored=_bf16_stored,
    past_B=lambda l3: {"a1": E.HW * E.C1, "dz1": E.HW * E.C1, "a2": E.HW * E.C2, "dz2": E.HW * E.C2, "dlogits": E.NO,
                       "loss_rows": 1},
    check_setup=lambda eng: None, check_plan=lambda eng, B, plan: None, check_stages=_bf16_stages)


def _fp32_stored(level, l3):
    stored = ["a2", "dz2", "w2slab", "w1slab", "loss_hist"]
    stored += ["dlogits", "loss_rows"] if l3 else ["fc_part"]  # level 3: granules; level 1: dL stays in LDS
    return stored


def _fp32_setup(eng):
    assert eng.dtype == "fp32" and eng.store_a1 == 0 and eng.opts.pxt_fwd == 2 and "a1" not in eng.t


def _fp32_plan(eng, B, plan):
    from ddp_amd.ops.functional import wgrad_rows

    assert eng.wgrad_rows == wgrad_rows(28, eng.B, torch.float32)
    # the row counts the reference derives are the launchers'
    nRC = -(-28 // eng.wgrad_rows)
    assert eng.C.conv3x3_wgrad_blocks(B, 28, eng.wgrad_rows) == B * nRC
    assert eng.C.conv3x3_dgrad_blocks(B, 28, 28, eng.opts.pxt_dgrad) == -(-B * E.HW // plan["CH1"])


def _fp32_stages(res, stored, level, mom, fuse_opt):
    want = E.fp32_stages(level, mom) - ({"grad_wfc"} if fuse_opt else set())
    assert set(res) == want, sorted(want ^ set(res))


FP32 = Precision(
    prec="fp32", tag="fp32",
    poison=("a2", "dz2", "fc_part", "dlogits", "loss_rows", "w2slab", "w1slab"),
    shadows=("w2t_f32", "wfc_frag32"),
    compute_dtype=torch.float32, options=dict(dtype="fp32"),
    stored=_fp32_stored,
    past_B=lambda l3: {"a2": E.HW * E.C2, "dz2": E.HW * E.C2, **({"dlogits": E.NO, "loss_rows": 1} if l3 else {})},
    check_setup=_fp32_setup, check_plan=_fp32_plan, check_stages=_fp32_stages)


def setup(p, n=256, B=32, momentum=0.0, weight_decay=0.0, use_graph=False, graph_steps=5, **eo):
    from ddp_amd.data import DeviceMNIST, synthetic_mnist
    from ddp_amd.engine import EngineOptions, FusedSimpleCNNEngine
    from ddp_amd.models import SimpleCNN
    from ddp_amd.ops import FusedSGD

    torch.manual_seed(0)
    model = (SimpleCNN() if p.compute_dtype is None else SimpleCNN(compute_dtype=p.compute_dtype)).to(dev)
    opt = FusedSGD(model, lr=LR, momentum=momentum, weight_decay=weight_decay)
    imgs, labels = synthetic_mnist(n)
    eng = FusedSimpleCNNEngine(model, opt, DeviceMNIST(imgs, labels, dev), B, 1, 0,
                               opts=EngineOptions(graph_steps=graph_steps, use_graph=use_graph, **{**p.options, **eo}))
    eng.refresh()
    p.check_setup(eng)
    return eng, imgs, labels


def begin(eng, epoch=0):
    eng.sync_from_torch()
    eng.start_epoch(epoch)


def by_name(eng, flat):
    return {k: eng.fs.view(flat, v).detach().cpu().clone() for k, v in NAMES.items()}


def checked_step(p, eng, imgs, labels, B, chain, first_step=False):
    """Snapshot, poison, one eager step of B images, check_step on what the chain materialises."""
    t, level, mom = eng.t, int(eng.cfg["fuse_level"]), eng.cfg["momentum"] != 0.0
    eng.synchronize()
    torch.cuda.synchronize()
    k = int(t["step_ctr"].item())
    before = by_name(eng, eng.fs.params)
    obs = {s: t[s].cpu().clone() for s in p.shadows}
    obs["loss_hist_before"] = t["loss_hist"].cpu().clone()
    if mom and not first_step:
        obs["momentum_before"] = by_name(eng, t["momentum"])
    idx = eng.sampler.indices()[k * eng.B:k * eng.B + B]
    assert idx.numel() == B
    for s in p.poison:
        t[s].fill_(float("nan"))
    for v in NAMES.values():  # (the views, not the alignment gaps the flat SGD kernel also sweeps)
        eng.fs.view(eng.fs.grads, v).fill_(float("nan"))
    torch.cuda.synchronize()
    eng.eng.step(B, eng.B)
    eng.synchronize()
    torch.cuda.synchronize()
    assert eng.eng.sync_error == 0
    assert int(t["step_ctr"].item()) == k + 1
    l3 = bool(eng.eng.last_level3)
    assert l3 == (level >= 3)
    stored = p.stored(level, l3)
    obs.update({s: t[s].cpu().clone() for s in stored})
    grads = by_name(eng, eng.fs.grads)
    if eng.cfg["fuse_opt"]:  # the fused optimizer consumes the fc weight gradient in registers
        assert bool(torch.isnan(grads.pop("wfc")).all())
    obs["grads"] = grads
    obs["params_after"] = by_name(eng, eng.fs.params)
    if mom:
        obs["momentum_after"] = by_name(eng, t["momentum"])
    g = eng.opt.param_groups[0]
    plan = E.make_plan(B, level=level, pxt_fwd=eng.opts.pxt_fwd, pxt_dgrad=eng.opts.pxt_dgrad, wgrad_rows=eng.wgrad_rows,
                       max_batch=eng.B, k=k, lr=g["lr"], momentum=g["momentum"], dampening=g["dampening"],
                       weight_decay=g["weight_decay"], nesterov=g["nesterov"], first_step=first_step, prec=p.prec)
    p.check_plan(eng, B, plan)
    res = E.check_step(obs, before, imgs[idx], labels[idx], B, plan)
    E.report(res, f"{p.tag}_{chain}" if p.tag else chain, B)
    bad = E.failing(res)
    who = f"{p.tag} {chain}" if p.tag else chain
    assert not bad, f"{who} B={B} step {k}: out of bound at {[(s, res[s]) for s in bad]}"
    p.check_stages(res, stored, level, mom, eng.cfg["fuse_opt"])
    if B < eng.B:  # a ragged batch leaves the rows past B alone
        for s, n in p.past_B(l3).items():
            assert bool(torch.isnan(t[s].reshape(-1)[B * n:].float()).all()), f"{who}: {s} written past row {B}"
    return res
