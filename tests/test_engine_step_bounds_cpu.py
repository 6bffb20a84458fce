"""CPU side of tests/test_engine_step_elementwise_gpu.py (no GPU needed): the staged checker of
tests/engine_step_cases.py admits a correct step and rejects wrong ones, each at its stage.

Admits: ``emulate_step`` - an fp32 / bf16 model of the engine's stage outputs, torch's float32
operators in another summation order than the float64 references - stays inside every
a-priori bound at B = 1, 3, 20, 32 and at an 8-image tail of max_batch = 64, on the first step
and on a later one (momentum, weight decay, another loss slot, another window of the index
list).  Evidence about the bounds and the checker, not about the engine.

Rejects: from that emulation, eight planted errors of the kind launch_step_t's wiring can make;
each must fail, and the first stage to fail (in dependency order) must be the one the error
belongs to.  A case only counts because the unmodified emulation passes the same check.
"""
import functools

import pytest
import torch

import engine_step_cases as E
from ddp_amd.ops import reference as R


@functools.lru_cache(maxsize=None)
def base(B, max_batch=None, k=0, momentum=0.0, wd=0.0):
    """(before, x_u8, labels, plan, obs) of a correct emulated step.  Shared: do not write."""
    imgs, labels, perm = E.dataset()
    mb = max_batch or B
    idx = perm[k * mb:k * mb + B]
    plan = E.make_plan(B, max_batch=mb, pxt_fwd=1 if mb <= 32 else 2, k=k, momentum=momentum, weight_decay=wd,
                       first_step=k == 0)
    before = E.masters()
    mom = {n: torch.randn(E.SHAPES[n], generator=torch.Generator().manual_seed(5)) * 0.01 for n in E.PARAMS} if k else None
    hist = torch.rand(k + 3) if k else None
    obs = E.emulate_step(before, imgs[idx], labels[idx], B, plan, momentum_before=mom, loss_hist_before=hist)
    return before, imgs[idx], labels[idx], plan, obs


def assert_passes(res, what):
    bad = E.failing(res)
    assert not bad, f"{what}: out of bound at {[(s, res[s]) for s in bad]}"


@pytest.mark.parametrize("B,max_batch,k,momentum,wd", [(1, None, 0, 0.0, 0.0), (3, None, 0, 0.9, 1e-4), (20, None, 0, 0.0, 0.0),
                                                       (32, None, 0, 0.9, 1e-4), (8, 64, 0, 0.0, 0.0), (3, None, 2, 0.9, 1e-4)])
def test_checker_admits_the_emulated_step(B, max_batch, k, momentum, wd):
    before, x, y, plan, obs = base(B, max_batch, k, momentum, wd)
    res = E.check_step(obs, before, x, y, B, plan)
    E.report(res, "cpu_emulation", B, tag="CPU_STEP_RATIO")
    assert_passes(res, f"emulation B={B}")
    # every stage of the table ran
    want = set(E.STAGES) if momentum else {s for s in E.STAGES if not s.startswith("momentum_")}
    assert set(res) == want


def test_emulation_keeps_reproducing_the_whole_step_reference():
    """emulate_step is R.simple_cnn_step_bf16 with the intermediates kept (per-block partial
    logits, slab rows): the same roundings at the same store points, so its gradients and loss
    agree with it to fp32 summation order."""
    before, x, y, plan, obs = base(3)
    loss, g = R.simple_cnn_step_bf16(before, x.float() / 255.0, y)
    for k in g:
        torch.testing.assert_close(obs["grads"][k].reshape(g[k].shape), g[k], rtol=1e-4, atol=1e-4 * g[k].abs().max().item())
    torch.testing.assert_close(obs["loss_hist"][0], loss, rtol=1e-6, atol=1e-6)


def first_failure(obs, before, x, y, B, plan):
    res = E.check_step(obs, before, x, y, B, plan)
    bad = E.failing(res)
    assert bad, "the planted error passed every stage"
    return bad[0], bad


def test_rejects_an_image_left_out_of_every_gradient_sum():
    before, x, y, plan, _ = base(3)
    obs = E.emulate_step(before, x, y, 3, plan, drop_image=1)
    first, bad = first_failure(obs, before, x, y, 3, plan)
    assert first == "grad_wfc", bad
    assert {"grad_wfc", "grad_bfc", "grad_w2", "grad_b2", "grad_w1", "grad_b1"} <= set(bad), bad
    assert not {"a1", "a2", "dlogits", "dz2", "dz1", "w2slab", "w1slab"} & set(bad), bad


def test_rejects_the_full_batch_scale_on_a_ragged_tail():
    before, x, y, plan, _ = base(8, 64)
    obs = E.emulate_step(before, x, y, 8, plan, gscale=1.0 / 64)
    first, bad = first_failure(obs, before, x, y, 8, plan)
    assert first == "dlogits", bad
    # teacher-forced: what follows the wrong dL is consistent with it
    assert not {"dz2", "dz1", "grad_wfc", "grad_w2", "grad_w1"} & set(bad), bad


def test_rejects_a_batch_gathered_one_index_late():
    imgs, labels, perm = E.dataset()
    before, x, y, plan, _ = base(3)
    late = perm[1:4]
    obs = E.emulate_step(before, imgs[late], labels[late], 3, plan)
    first, bad = first_failure(obs, before, x, y, 3, plan)
    assert first == "a1", bad


def test_rejects_one_bias_gradient_element_at_four_bounds():
    before, x, y, plan, obs = base(3)
    res = E.check_step(obs, before, x, y, 3, plan)
    assert_passes(res, "emulation")
    # the bound of grad_bfc[7], recovered from the float64 reference the checker used
    _, _, gref = R.fc_bwd64(obs["dlogits"], obs["a2"], E.bf(before["wfc"]), 1.0, False)
    _, _, Ab = R.fc_bwd64(obs["dlogits"].abs(), obs["a2"].abs(), E.bf(before["wfc"]), 1.0, False)
    bound = E.acc_bound(3 + 2, Ab)
    bumped = dict(obs, grads=dict(obs["grads"]))
    bumped["grads"]["bfc"] = (gref + 4 * bound * (torch.arange(10) == 7)).float()
    res = E.check_step(bumped, before, x, y, 3, plan)
    bad = E.failing(res)
    assert bad[0] == "grad_bfc" and res["grad_bfc"][1] == (7,), (bad, res["grad_bfc"])
    assert 2.0 < res["grad_bfc"][0] < 6.0
    # (the parameters were updated with the gradient the emulation computed, not the moved one)
    assert set(bad) <= {"grad_bfc", "param_bfc"}, bad


def test_rejects_a_conv2_shadow_one_step_stale():
    before0, x, y, plan, obs0 = base(3)
    after0 = obs0["params_after"]
    plan1 = dict(plan, k=1)
    obs = E.emulate_step(after0, x, y, 3, plan1)
    assert_passes(E.check_step(obs, after0, x, y, 3, plan1), "second step")
    stale = dict(obs, w2_bf16=E.entry_shadows(before0)["w2_bf16"])
    assert not torch.equal(E.bits(stale["w2_bf16"]), E.bits(obs["w2_bf16"]))
    first, bad = first_failure(stale, after0, x, y, 3, plan1)
    assert first == "shadows" and bad == ["shadows"], bad


def test_rejects_a_slab_row_left_out_of_the_reduction():
    before, x, y, plan, _ = base(20)
    rows = 20 * -(-28 // plan["R"])
    assert plan["R"] == 4 and rows == 140  # what wgrad_rows(28, 20) gives: the 16-group reducer
    obs = E.emulate_step(before, x, y, 20, plan, drop_w2_row=rows - 1)  # the last row: B = 20's own count
    first, bad = first_failure(obs, before, x, y, 20, plan)
    assert first == "grad_w2", bad
    assert "w2slab" not in bad and "grad_w1" not in bad, bad


def test_rejects_a_loss_written_one_slot_late():
    before, x, y, plan, _ = base(3, None, 2, 0.9, 1e-4)
    hist = torch.rand(5)
    mom = {n: torch.zeros(E.SHAPES[n]) for n in E.PARAMS}
    obs = E.emulate_step(before, x, y, 3, plan, momentum_before=mom, loss_hist_before=hist, hist_slot=3)
    first, bad = first_failure(obs, before, x, y, 3, plan)
    assert first == "loss_hist" and bad == ["loss_hist"], bad


def test_rejects_a_dz2_element_where_the_activation_is_zero():
    before, x, y, plan, obs = base(3)
    zero = torch.nonzero(obs["a2"].float() == 0)
    assert zero.numel()
    i = tuple(int(v) for v in zero[len(zero) // 2])
    leak = dict(obs, dz2=obs["dz2"].clone())
    leak["dz2"][i] = 2.0 ** -30
    res = E.check_step(leak, before, x, y, 3, plan)
    bad = E.failing(res)
    assert bad[0] == "dz2" and res["dz2"][1] == i, (bad, res["dz2"])


def test_carried_bounds_admit_the_chains_that_store_less():
    """Level >= 1 keeps dZ1 in registers and level 1 keeps dL and the row losses in LDS: without
    them the checker carries the float64 value's bound forward - and still sees an image left
    out of the conv1 gradient or a wrong cross-entropy scale."""
    before, x, y, plan, obs = base(3)
    for drop in (("dz1",), ("dz1", "dlogits", "loss_rows"), ("dz1", "dlogits", "loss_rows", "fc_part")):
        less = {k: v for k, v in obs.items() if k not in drop}
        res = E.check_step(less, before, x, y, 3, plan)
        assert_passes(res, f"without {drop}")
        assert not set(drop) & set(res)
    bad_obs = E.emulate_step(before, x, y, 3, plan, drop_image=2)
    less = {k: v for k, v in bad_obs.items() if k not in ("dz1", "dlogits", "loss_rows")}
    bad = E.failing(E.check_step(less, before, x, y, 3, plan))
    assert {"grad_wfc", "grad_bfc", "grad_w1", "grad_b1"} <= set(bad), bad
    bad_obs = E.emulate_step(before, x, y, 3, plan, gscale=1.0 / 4)
    less = {k: v for k, v in bad_obs.items() if k not in ("dz1", "dlogits", "loss_rows")}
    assert E.failing(E.check_step(less, before, x, y, 3, plan))[0] == "dz2"
