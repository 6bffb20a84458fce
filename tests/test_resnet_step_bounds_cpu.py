"""CPU side of tests/test_resnet_step_elementwise_gpu.py (no GPU needed): the staged checker of
tests/resnet_step_cases.py admits a correct ResNet-18 step and rejects wrong ones, each at its
stage.

Admits: ``emulate_forward_backward`` / ``emulate_sgd`` - an fp32 / bf16 model of the step that
follows the case file's own topology (torch's float32 operators, another summation order than the
float64 references) - stays inside every a-priori bound for ``s64`` (two steps), ``s72`` and
``accum``.  Evidence about the bounds and the checker, not about the kernels.

Rejects: thirteen planted wiring errors; each must fail, and the first stage to fail (in
dependency order) must be the one the error belongs to.  Only the affected layers are re-checked
(``only=``); a case counts because the unmodified emulation passes the full check.
"""
import functools

import pytest
import torch

import resnet_step_cases as S


def _ctx(P, img, labels, cs, nbt, first, layout=None, prior=None, grads_before=None):
    return dict(params={k: v.clone() for k, v in P.items()}, image=img, labels=labels,
                label_smoothing=cs["label_smoothing"], nbt=nbt, prior=prior, layout=layout, hp=S.HP,
                first_step=first, grads_before=grads_before)


@functools.lru_cache(maxsize=None)
def run_case(case, plant=None):
    """[(trace, ctx, backwards)] per optimizer step of an emulated case.  Shared: do not write."""
    cs = S.CASES[case]
    P, Bf = S.make_model(cs["classes"])
    grads, mom, out, nbt = {}, None, [], 0
    for step in range(cs["steps"]):
        T, prior, micro = [], None, cs.get("micro", 1)
        for mb in range(micro):
            img, labels = S.make_batch(cs["B"], cs["size"], cs["classes"], seed=10 * step + mb)
            if mb == micro - 1 and mb > 0:
                prior = {k: v.clone() for k, v in grads.items()}
            # a new step overwrites (lazy zero_grad); a further micro-batch adds
            over = mb == 0 and not (plant == "accumulate_second_step" and step == 1)
            p = plant if plant != "accumulate_second_step" else None
            T += S.emulate_forward_backward(P, Bf, img, labels, grads, nbt, cs["label_smoothing"], overwrite=over, plant=p)
            nbt += 1
        call, lay, newP, newM = S.emulate_sgd(P, grads, mom, S.HP, step == 0, plant=plant)
        out.append((T + [call], _ctx(P, img, labels, cs, nbt - 1, step == 0, lay, prior), micro))
        P, mom = newP, newM
    return out


@pytest.mark.parametrize("case", ["s64", "s72", "accum"])
def test_checker_admits_the_emulated_step(case):
    for k, (trace, ctx, backwards) in enumerate(run_case(case)):
        res = S.check_step(trace, ctx, backwards)
        S.report(res, f"cpu_emulation_{case}_step{k}", tag="CPU_RESNET_STEP_RATIO")
        bad = S.failing(res)
        assert not bad, f"{case} step {k}: out of bound at {[(s, res[s]) for s in bad]}"
        assert set(res) == set(S.STAGES), set(S.STAGES) ^ set(res)  # every stage of the table ran


def test_emulated_cases_reach_both_weight_gradient_paths():
    trace, _, _ = run_case("s64")[0]
    sts, _ = S.parse_trace(trace)
    reds = [n for n, b in sts[0]["bwd"].items() if b["red"] is not None]
    assert reds and len(reds) < 20, reds


def test_topology_is_resnet18():
    t = S.TOPO
    assert len(t["convs"]) == 20 and len(t["blocks"]) == 8 and sum(b["ds"] for b in t["blocks"]) == 3
    assert [c["s"] for c in t["convs"] if c["role"] == "conv1"] == [1, 1, 2, 1, 2, 1, 2, 1]
    assert len(S.param_names()) == 62
    # identity blocks sum conv1's dx with bn2's dres, downsample blocks with the 1x1 conv's dx
    assert t["grad"]["layer1.0.conv2"] == (("dx", "layer1.1.conv1"), ("dres", "layer1.1.conv2"))
    assert t["grad"]["layer1.1.conv2"] == (("dx", "layer2.0.conv1"), ("dx", "layer2.0.downsample.0"))
    assert t["grad"]["layer4.1.conv2"] == (("avgpool", None), None)


# plant -> (step of s64, layers re-checked, optimizer landing re-checked, first failing stage)
REJECT = {
    "res_from_conv1": (0, {"layer1.1.conv2"}, False, "bn_apply"),
    "stash_dropped": (0, {"layer1.0.conv2"}, False, "bn_bwd_dres"),
    "stash_twice": (0, {"layer1.0.conv2"}, False, "bn_bwd_dres"),
    "relu_after_ds": (0, {"layer2.0.downsample.0"}, False, "bn_apply"),
    "biased_var": (0, {"layer3.0.conv1"}, False, "running_var"),
    "momentum_swapped": (0, {"layer3.0.conv1"}, False, "running_mean"),
    "dgamma_dbeta_swapped": (0, {"layer2.1.conv1"}, False, "bn_dgamma"),
    "wgrad_wrong_slot": (0, set(), True, "landing"),
    "accumulate_second_step": (1, {"head", "layer4.1.conv2", "conv1"}, False, "head_dw"),
    "no_1_over_B": (0, {"head"}, False, "dlogits"),
    "mask_pre_residual": (0, {"layer1.1.conv2"}, False, "bn_bwd_dres"),
    "pad4_nonzero": (0, {"conv1"}, False, "pad4"),
    "nbt_stuck": (0, {"layer1.0.conv1"}, False, "nbt"),
}


def test_every_planted_error_has_a_case():
    assert set(REJECT) == set(S.PLANTS)


@pytest.mark.parametrize("plant", S.PLANTS)
def test_checker_rejects_at_the_stage(plant):
    step, only, landing, stage = REJECT[plant]
    # the correct emulation passes the very same restricted check
    trace, ctx, backwards = run_case("s64")[step]
    good = S.check_step(trace, ctx, backwards, only=only, optimizer=landing)
    assert not S.failing(good), (plant, S.failing(good))
    trace, ctx, backwards = run_case("s64", plant)[step]
    res = S.check_step(trace, ctx, backwards, only=only, optimizer=landing)
    bad = S.failing(res)
    assert bad and bad[0] == stage, (plant, [(s, res[s]) for s in bad])
    if plant == "accumulate_second_step":
        assert {"head_dw", "head_db", "bn_dgamma", "bn_dbeta", "wgrad"} <= set(bad), bad
    if plant == "stash_dropped":
        assert res["bn_bwd_dres"][1][0] == "layer1.0.bn2"
    if plant == "wgrad_wrong_slot":
        assert res["landing"][1][0] == "layer1.0.conv1.weight"


def test_a_missing_or_extra_call_names_the_layer():
    trace, ctx, backwards = run_case("s64")[0]
    i = next(k for k, c in enumerate(trace) if c.name == "conv_gemm_dgrad")
    res = S.check_step(trace[:i] + trace[i + 1:], ctx, backwards, only=set(), optimizer=False)
    assert S.failing(res) == ["order"] and "layer4.1.conv2 data gradient" in res["order"][1][0], res
    j = max(k for k, c in enumerate(trace) if c.name == "conv_gemm_wgrad")
    extra = trace[:j] + [S.Call("conv_gemm_dgrad", trace[i].a, trace[i].o)] + trace[j:]
    res = S.check_step(extra, ctx, backwards, only=set(), optimizer=False)  # a dgrad for the stem
    assert S.failing(res) == ["order"] and "conv1 weight gradient" in res["order"][1][0], res


def test_bn_finalize_bound_shows_the_cancellation():
    """mean 8, deviation 2**-6: the invstd bound is a few per cent of invstd (3 u m^2 / v = 4.7 %
    of the variance), a channel of mean 0 a few u - and an fp32 evaluation stays inside both."""
    n = 64
    x = torch.empty(n, 2, dtype=torch.float64)
    x[:, 0] = 8.0 + 2.0 ** -6 * (1 - 2 * (torch.arange(n) % 2))
    x[:, 1] = 2.0 ** -6 * (1 - 2 * (torch.arange(n) % 2))
    slab = torch.stack([x.sum(0), (x * x).sum(0)]).float().view(1, 2, 2)
    b = S.bn_finalize_bounds(slab, n, 1e-5, 0.1)
    ref, bound = b["invstd"]
    rel = bound / ref
    assert 0.02 < rel[0] < 0.2 and rel[1] < 16 * S.U, rel
    mean = slab[0, 0] / n
    var = (slab[0, 1] / n - mean * mean).clamp(min=0)
    inv = (var + 1e-5).rsqrt()
    assert bool(((inv.double() - ref).abs() <= bound).all())
