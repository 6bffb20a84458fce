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

The second half does the same for the exact-fp32 table (``prec="fp32"``,
tests/test_engine_step_fp32_elementwise_gpu.py): the fp32 emulation is admitted at the same sizes
on both stored-stage sets (level 1, level 3); the wiring errors above, a bf16-rounded weight, a
wrong w2t_f32, a wrong channel half of a slab row, a conv1 mask flipped outside the ambiguous
set and a reduced gradient one ulp off the replay are rejected at their stages; a mask flipped
inside the ambiguous set is admitted; and the ambiguous share stays under its cap for every
batch the GPU file gathers.
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


# ------------------------------------------------------------------ the exact-fp32 table
# The same for prec="fp32" (tests/test_engine_step_fp32_elementwise_gpu.py): the emulation has
# no bf16 rounding and leaves a1 and dz1 out; every bound is 3 n u A.
@functools.lru_cache(maxsize=None)
def base32(B, max_batch=None, k=0, momentum=0.0, wd=0.0):
    """(before, x_u8, labels, plan, obs) of a correct emulated fp32 step.  Shared: do not write."""
    imgs, labels, perm = E.dataset()
    mb = max_batch or B
    idx = perm[k * mb:k * mb + B]
    plan = E.make_plan(B, level=3, max_batch=mb, k=k, momentum=momentum, weight_decay=wd, first_step=k == 0, prec="fp32")
    before = E.masters()
    mom = {n: torch.randn(E.SHAPES[n], generator=torch.Generator().manual_seed(5)) * 0.01 for n in E.PARAMS} if k else None
    hist = torch.rand(k + 3) if k else None
    obs = E.emulate_step(before, imgs[idx], labels[idx], B, plan, momentum_before=mom, loss_hist_before=hist)
    return before, imgs[idx], labels[idx], plan, obs


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("B,max_batch,k,momentum,wd", [(1, None, 0, 0.0, 0.0), (3, None, 0, 0.9, 1e-4), (20, None, 0, 0.0, 0.0),
                                                       (32, None, 0, 0.9, 1e-4), (8, 64, 0, 0.0, 0.0), (3, None, 2, 0.9, 1e-4)])
def test_fp32_checker_admits_the_emulated_step(B, max_batch, k, momentum, wd, level):
    before, x, y, plan, obs = base32(B, max_batch, k, momentum, wd)
    assert plan["CH"] == 128 and plan["R"] == {1: 1, 3: 1, 20: 4, 32: 4, 8: 4}[B]
    assert "a1" not in obs and "dz1" not in obs and obs["a2"].dtype == torch.float32
    res = E.check_step(E.stored_on(obs, level), before, x, y, B, plan)
    E.report(res, f"cpu_emulation_fp32_l{level}", B, tag="CPU_STEP_RATIO")
    assert_passes(res, f"fp32 emulation B={B} level {level}")
    assert set(res) == E.fp32_stages(level, momentum)  # every stage of the fp32 table ran


def first32(level, B=3, max_batch=None, **errors):
    before, x, y, plan, _ = base32(B, max_batch)
    obs = E.stored_on(E.emulate_step(before, x, y, B, plan, **errors), level)
    return first_failure(obs, before, x, y, B, plan)


def test_fp32_rejects_the_wiring_errors_of_the_bf16_table():
    first, bad = first32(3, drop_image=1)
    assert first == "grad_wfc" and {"grad_wfc", "grad_bfc", "grad_w2", "grad_b2", "grad_w1", "grad_b1"} <= set(bad), bad
    assert not {"a2", "dlogits", "dz2", "w2slab", "w1slab"} & set(bad), bad
    first, bad = first32(3, gscale=1.0 / 4)
    assert first == "dlogits" and not {"dz2", "grad_wfc", "grad_w2", "grad_w1"} & set(bad), bad
    assert first32(1, gscale=1.0 / 4)[0] == "dz2"  # (level 1 carries dL: seen where it is first stored)
    first, bad = first32(3, B=20, drop_w2_row=20 * 7 - 1)
    assert first == "grad_w2" and "w2slab" not in bad and "grad_w1" not in bad, bad
    before, x, y, plan, _ = base32(3, None, 2, 0.9, 1e-4)
    mom = {n: torch.zeros(E.SHAPES[n]) for n in E.PARAMS}
    obs = E.emulate_step(before, x, y, 3, plan, momentum_before=mom, loss_hist_before=torch.rand(5), hist_slot=3)
    first, bad = first_failure(E.stored_on(obs, 3), before, x, y, 3, plan)
    assert first == "loss_hist" and bad == ["loss_hist"], bad


def test_fp32_rejects_the_full_batch_scale_on_a_ragged_tail():
    first, bad = first32(3, B=8, max_batch=64, gscale=1.0 / 64)
    assert first == "dlogits" and not {"dz2", "grad_wfc", "grad_w2", "grad_w1"} & set(bad), bad


def test_fp32_bounds_are_tighter_than_a_bf16_rounding_of_the_weights():
    """A bf16 build wired into the fp32 chain: conv2's weight rounded to bf16 fails at a2, the fc
    weight at the first stored stage that reads it - the partial logits on level 1; on level 3,
    which stores no partials, dZ2 (a whole logit's 50176 rounded terms average out far below
    any worst-case bound of their sum; dZ2's 10 do not)."""
    for level in (1, 3):
        first, bad = first32(level, bf16_w2=True)
        assert first == "a2", bad
    first, bad = first32(1, bf16_wfc=True)
    assert first == "fc_part" and "a2" not in bad, bad
    first, bad = first32(3, bf16_wfc=True)
    assert first == "dz2" and "a2" not in bad, bad


def test_fp32_rejects_a_wrong_conv2_weight_copy():
    first, bad = first32(3, w2t="plain")
    assert first == "shadows" and "w1slab" in bad and "a2" not in bad, bad  # (the dgrad read it)
    before0, x, y, plan, obs0 = base32(3)
    after0 = obs0["params_after"]
    plan1 = dict(plan, k=1)
    obs = E.emulate_step(after0, x, y, 3, plan1)
    assert_passes(E.check_step(E.stored_on(obs, 3), after0, x, y, 3, plan1), "second step")
    stale = E.stored_on(E.emulate_step(after0, x, y, 3, plan1, w2t=before0), 3)
    assert not torch.equal(E.bits(stale["w2t_f32"]), E.bits(obs["w2t_f32"]))
    first, bad = first_failure(stale, after0, x, y, 3, plan1)
    assert first == "shadows", bad


@pytest.mark.parametrize("error", ["zero_w2_half", "borrow_w2_half"])
def test_fp32_rejects_a_wrong_channel_half_of_a_conv2_slab_row(error):
    """The second block of a row (ci 16..31) did not write, or wrote the row next to its own."""
    before, x, y, plan, obs = base32(3)
    first, bad = first32(3, **{error: 40})
    assert first == "w2slab" and "w1slab" not in bad, bad
    res = E.check_step(E.stored_on(E.emulate_step(before, x, y, 3, plan, **{error: 40}), 3), before, x, y, 3, plan)
    assert res["w2slab"][1][0] == 40 and res["w2slab"][1][1] % E.C1 >= 16 and res["w2slab"][1][1] < E.N_W2, res["w2slab"]
    # the reduced gradient is still the replay of the rows that were stored
    assert res["replay_w2"][0] == 0.0 and res["grad_w2"][0] > 1.0


def test_fp32_rejects_the_conv1_channel_halves_of_a_w1_slab_row_swapped():
    first, bad = first32(3, swap_w1_halves=5)
    assert first == "w1slab" and "w2slab" not in bad, bad


def test_fp32_rejects_a_reduced_gradient_one_ulp_off_the_replay():
    before, x, y, plan, obs = base32(3)
    off = dict(E.stored_on(obs, 3), grads=dict(obs["grads"]))
    off["grads"]["b1"] = obs["grads"]["b1"].clone()
    off["grads"]["b1"][7] = torch.nextafter(off["grads"]["b1"][7], torch.tensor(float("inf")))
    res = E.check_step(off, before, x, y, 3, plan)
    assert E.failing(res) == ["replay_b1"], E.failing(res)


def _ambiguous_case():
    """Masters whose b1[5] is moved so that one conv1 pre-activation is (to the rounding of b1
    itself, within e_a1) zero: an ambiguous element exists."""
    before, x, y, plan, _ = base32(3)
    pre = R.conv1_64(x, before["w1"].reshape(E.C1, 9), before["b1"], relu=False)
    nz = torch.nonzero((x[1] > 0) & (pre[1, :, :, 5] != before["b1"][5].double()))
    h, w = (int(v) for v in nz[len(nz) // 2])
    moved = dict(before, b1=before["b1"].clone())
    moved["b1"][5] = (before["b1"][5].double() - pre[1, h, w, 5]).float()
    return moved, x, y, plan, (1, h, w, 5)


def test_fp32_conv1_mask_flip_passes_inside_the_ambiguous_set_and_fails_outside_it():
    moved, x, y, plan, at = _ambiguous_case()
    pre = R.conv1_64(x, moved["w1"].reshape(E.C1, 9), moved["b1"], relu=False)
    A = R.conv3x3_64((x.double() / 255.0).unsqueeze(-1), moved["w1"].double().abs(), moved["b1"].double().abs())
    amb = pre.abs() <= E.acc_bound(11, A, True)
    assert bool(amb[at]) and amb.double().mean().item() <= E.AMBIG_CAP
    ok = E.stored_on(E.emulate_step(moved, x, y, 3, plan), 3)
    assert_passes(E.check_step(ok, moved, x, y, 3, plan), "moved bias")
    inside = E.stored_on(E.emulate_step(moved, x, y, 3, plan, flip_mask=at), 3)
    assert not torch.equal(inside["w1slab"], ok["w1slab"])  # (the flip changed a row)
    assert_passes(E.check_step(inside, moved, x, y, 3, plan), "a mask flipped inside the ambiguous set")
    # outside: the element of the same image and channel with the largest data gradient
    d = R.conv3x3_dgrad64(ok["dz2"], moved["w2"])[1, :, :, 5].abs() * ~amb[1, :, :, 5]
    h, w = divmod(int(d.reshape(-1).argmax()), E.W)
    outside = E.stored_on(E.emulate_step(moved, x, y, 3, plan, flip_mask=(1, h, w, 5)), 3)
    first, bad = first_failure(outside, moved, x, y, 3, plan)
    assert first == "w1slab" and "w2slab" not in bad, bad


def test_fp32_checker_refuses_more_ambiguous_masks_than_the_cap():
    before, x, y, plan, obs = base32(3)
    zeroed = dict(before, w1=torch.zeros_like(before["w1"]), b1=torch.zeros_like(before["b1"]))  # every pre-activation 0
    with pytest.raises(AssertionError, match="ambiguous"):
        E.check_step(E.stored_on(obs, 3), zeroed, x, y, 3, plan)


# the (n, B, max_batch, epoch, k) of every batch tests/test_engine_step_fp32_elementwise_gpu.py checks
GPU_BATCHES = [(256, B, B, 0, 0) for B in (1, 12, 20, 32, 40, 64)] + [(256, 32, 32, 0, 3), (256, 32, 32, 0, 6),
                                                                      (100, 4, 32, 0, 3), (100, 32, 32, 1, 0)]


@pytest.mark.parametrize("n,B,max_batch,epoch,k", GPU_BATCHES)
def test_fp32_ambiguous_masks_stay_under_the_cap_for_every_gpu_batch(n, B, max_batch, epoch, k):
    """The seed-0 model's conv1 on the window of the sampler's index list the GPU case gathers."""
    from ddp_amd.data import synthetic_mnist
    from ddp_amd.data.sampler import ShardedSampler
    from ddp_amd.models import SimpleCNN

    torch.manual_seed(0)
    m = SimpleCNN(compute_dtype=torch.float32)
    imgs, _ = synthetic_mnist(n)
    sampler = ShardedSampler(n, 1, 0, shuffle=True, seed=0)
    sampler.set_epoch(epoch)
    x = imgs[sampler.indices()[k * max_batch:k * max_batch + B]]
    assert x.shape == (B, 28, 28) and x.dtype == torch.uint8
    w1, b1 = m.net[0].weight.detach(), m.net[0].bias.detach()
    pre = R.conv1_64(x, w1.reshape(E.C1, 9), b1, relu=False)
    A = R.conv3x3_64((x.double() / 255.0).unsqueeze(-1), w1.double().abs().reshape(E.C1, 3, 3, 1), b1.double().abs())
    share = (pre.abs() <= E.acc_bound(11, A, True)).double().mean().item()
    print(f"AMBIGUOUS n={n} B={B} epoch={epoch} k={k} share {share:.2e}")
    assert share <= E.AMBIG_CAP
