"""LAMB on the CPU: the coefficient table against float64 closed forms, the torch-op step against
kernel_bounds.lamb_reference under its derived bounds, the state-dict round trips and the CLI's
refusals."""
import math

import numpy as np
import pytest
import torch

from ddp_amd.models import SimpleCNN
from ddp_amd.ops import FusedAdamW, FusedLAMB, LRSchedule
from ddp_amd.ops import kernel_bounds as kb
from ddp_amd.ops.lamb import lamb_coef_table

B1, B2 = 0.9, 0.95


def test_coef_table_entries_and_end_point():
    """Every entry is the float64 closed form rounded once; with a cosine schedule the table is as
    long as the schedule; without one it ends at the first step whose corrections both round to 1."""
    sched = LRSchedule(0.3, 40, "cosine", warmup_steps=4)
    tab = lamb_coef_table(0.3, (B1, B2), True, sched).numpy()
    short = lamb_coef_table(0.3, (B1, B2), True, None).numpy()
    one = lambda k: (np.float32(1 / (1 - B1 ** k)), np.float32(math.sqrt(1 - B2 ** k)))
    t_sat = next(t for t in range(10 ** 6) if one(t + 1) == (1.0, 1.0))
    assert len(short) == t_sat + 1 and len(tab) == max(40, t_sat + 1) and t_sat > 40
    for t, row in enumerate(tab):
        want = (*one(t + 1), np.float32(sched.lr_at(t)), np.float32(0))
        assert tuple(row) == want, (t, row, want)
    assert tuple(short[-1]) == (1.0, 1.0, np.float32(0.3), 0.0) and tuple(short[-2][:2]) != (1.0, 1.0)
    off = lamb_coef_table(0.3, (B1, B2), False, None).numpy()
    assert off.tolist() == [[1.0, 1.0, float(np.float32(0.3)), 0.0]]


def _model():
    torch.manual_seed(0)
    return SimpleCNN()


def _fill_grads(opt, seed):
    g = torch.Generator().manual_seed(seed)
    opt.flat.reattach_grads()
    for p in opt.model.parameters():
        p.grad.copy_(torch.randn(p.shape, generator=g) * 0.1)


def check_step(opt, k, w0, g0, m0, v0, eps, clip, torch_ops):
    """Step k + 1 of ``opt``, just taken from the flat float32 state (w0, g0, m0, v0), against the
    float64 rule: moments, parameters and ratios inside lamb_reference's bounds.  ``torch_ops`` (the
    CPU path): torch's add / addcmul round the product that the kernel's fma keeps exact - one more
    u per line, and 4 u on a ratio.  With clipping the step must really have been clipped."""
    fs = opt.flat
    wds, adapts = opt._seg_coefs()
    ibc1, bc2, lr, _ = opt.coef_table()[k].tolist()
    ref = kb.lamb_reference(w0, g0, m0, v0, [(fs.offsets[n], fs.numels[n]) for n in fs.names], wds, adapts, lr, B1, B2,
                            eps, ibc1, bc2, coef=opt.grad_clip_stats()["coef"] if clip else None)
    assert not clip or opt.grad_clip_stats()["clipped"] == k + 1, "the clip coefficient stayed 1"
    for got, key in ((opt.exp_avg, "m"), (opt.exp_avg_sq, "v"), (fs.params, "p")):
        err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref[key])
        assert (err <= ref["b" + key] + 2 * kb.U * torch_ops * np.abs(ref[key])).all(), (k, key, err.max())
    st = opt.trust_stats()
    for s, n in enumerate(fs.names):
        assert abs(st[n]["ratio"] - ref["phi"][s]) <= max(ref["rel_phi"][s], 4 * kb.U * torch_ops) * ref["phi"][s], (k, n)
        assert st[n]["adapted"] == adapts[s] and (adapts[s] or st[n]["ratio"] == 1.0)


@pytest.mark.parametrize("clip", [None, 0.5])
def test_cpu_step_against_reference(clip):
    """Three steps (bias correction moves), each against the float64 rule from the state before it."""
    opt = FusedLAMB(_model(), lr=0.05, betas=(B1, B2), eps=1e-6, weight_decay=0.1, max_grad_norm=clip)
    _fill_grads(opt, 1)
    fs = opt.flat
    assert 0 < sum(opt._seg_coefs()[1]) < len(fs.names)
    state = [np.zeros(fs.numel, np.float32)] * 2
    for k in range(3):
        before = [fs.params.detach().numpy().copy(), fs.grads.numpy().copy(), *state]
        opt.step()
        check_step(opt, k, *before, 1e-6, clip, True)
        state = [opt.exp_avg.numpy().copy(), opt.exp_avg_sq.numpy().copy()]
    assert opt.schedule_step() == 3


def test_state_dict_round_trips():
    lamb = FusedLAMB(_model(), lr=0.05, betas=(B1, B2), weight_decay=0.1, exclude=None, bias_correction=False)
    _fill_grads(lamb, 2)
    lamb.step()
    lamb.step()
    sd = lamb.state_dict()
    g = sd["param_groups"][0]
    assert g["exclude"] is None and g["bias_correction"] is False and g["betas"] == (B1, B2)
    adam = FusedAdamW(SimpleCNN(), lr=0.1)
    adam.load_state_dict(sd)
    assert torch.equal(adam.exp_avg, lamb.exp_avg) and torch.equal(adam.exp_avg_sq, lamb.exp_avg_sq)
    assert adam.state_counter() == 2 and adam.param_groups[0]["betas"] == (B1, B2) and "exclude" not in adam.param_groups[0]
    params = [torch.nn.Parameter(torch.zeros_like(s["exp_avg"])) for s in sd["state"].values()]
    topt = torch.optim.AdamW(params, lr=0.1)
    topt.load_state_dict(sd)
    assert torch.equal(topt.state[params[0]]["exp_avg"], sd["state"][0]["exp_avg"])
    assert float(topt.state[params[0]]["step"]) == 2.0
    back = FusedLAMB(SimpleCNN(), lr=0.1)
    back.load_state_dict(adam.state_dict())  # no LAMB keys in FusedAdamW's dict: the constructor's stay
    assert torch.equal(back.exp_avg, lamb.exp_avg) and back.state_counter() == 2
    assert back.param_groups[0]["exclude"] == "1d" and back.param_groups[0]["bias_correction"] is True
    back.load_state_dict(topt.state_dict())  # torch hands the extra keys through
    assert torch.equal(back.exp_avg_sq, lamb.exp_avg_sq) and back.state_counter() == 2
    assert back.param_groups[0]["exclude"] is None and back.param_groups[0]["bias_correction"] is False
    assert FusedLAMB(SimpleCNN(), exclude=lambda n, s: False).state_dict()["param_groups"][0]["exclude"] == "callable"


def test_cli_refusals():
    from ddp_amd.engine.trainer import TrainOptions, check_fused_engine_options, validate_options

    with pytest.raises(ValueError, match="--optimizer lamb takes --beta1"):
        validate_options(TrainOptions(optimizer="lamb", momentum=0.9))
    with pytest.raises(ValueError, match="--optimizer lamb needs the module path"):
        check_fused_engine_options(TrainOptions(optimizer="lamb"), True)
    validate_options(TrainOptions(optimizer="lamb", lars_exclude="none", device="cpu"))
