"""CPU side of tests/test_simplecnn_step_elementwise_gpu.py (no GPU needed): the staged checker of
tests/simplecnn_step_cases.py admits a correct SimpleCNN module-path step and rejects wrong ones,
each at its stage.

Admits: ``emulate_case`` - an fp32 model of the step (torch's float32 operators, another summation
order than the float64 references; the bf16 rounding model for the bf16 cases, exact fp32 for the
fp32 ones) - stays inside every a-priori bound for every case the GPU file records.  Evidence
about the bounds and the checker, not about the kernels.

Rejects: fourteen planted wiring errors, one at a time, each on the smallest case that exposes
it; each must fail, and the first stage to fail (in dependency order) must be the one the error
belongs to.  A case counts because the unmodified emulation of the same case passes.
"""
import pytest
import torch

import simplecnn_step_cases as S
from ddp_amd.ops.functional import wgrad_rows


def test_cases_reach_every_wgrad_rows_branch():
    for (dt, B), Rr in S.WGRAD_ROWS.items():
        assert wgrad_rows(28, B, dt) == Rr, (dt, B)
        assert B == 1 or wgrad_rows(28, B - 1, dt) < Rr, (dt, B)  # the smallest batch of its branch
    have = {(cs["dtype"], B) for cs in S.CASES.values() for sizes in cs["steps"] for B in sizes}
    assert set(S.WGRAD_ROWS) <= have


def test_layout_is_reverse_registration_order_on_64_element_boundaries():
    lay, total = S.flat_layout()
    assert list(lay) == list(reversed(S.NAMES))
    assert lay["fl.bias"] == (0, 10) and lay["fl.weight"] == (64, 501760) and lay["net.2.bias"][0] == 64 + 501760
    assert all(off % 64 == 0 for off, _ in lay.values()) and total % 64 == 0
    assert int(S.inside_mask(lay, total).sum()) == 520586  # SimpleCNN's parameter count


@pytest.mark.parametrize("case", [c for c in S.CASES if c != "input_grad"])
def test_checker_admits_the_emulated_step(case):
    recs = S.emulate_case(case)
    assert len(recs) == len(S.CASES[case]["steps"])
    for k, rec in enumerate(recs):
        res = S.check_step(rec)
        S.report(res, f"cpu_emulation_{case}_step{k}", tag="CPU_SIMPLECNN_STEP_RATIO")
        bad = S.failing(res)
        assert not bad, f"{case} step {k}: out of bound at {[(s, res[s]) for s in bad]}"
        assert set(res) == set(S.STAGES) - {"input_grad"}, set(S.STAGES) ^ set(res)  # every stage of the table ran


# plant -> (case, step, first failing stage, stages that must fail too)
REJECT = {
    "nominal_batch": ("ragged", 1, "wire_xent", {"dlogits"}),
    "mask_from_a1": ("b1_bf16", 0, "wire_dgrad", set()),
    "wgrad_unmasked": ("b1_bf16", 0, "wire_wgrad", set()),
    "wt_swapped": ("b1_bf16", 0, "wire_dgrad", set()),
    "fc_nchw": ("b1_bf16", 0, "wire_fc", set()),
    "row_dropped": ("b1_bf16", 0, "gw2", {"gb2", "replay_w2", "replay_b2"}),
    "gb2_offset": ("b1_bf16", 0, "wire_red2", {"gb2", "replay_b2"}),
    "landing_shifted": ("b1_bf16", 0, "landing", set()),  # (64 elements on: the head of net.2.weight's view)
    "biases_swapped": ("b1_bf16", 0, "landing", set()),
    "accum_overwrites": ("accum", 0, "landing", set()),
    "no_half_scale": ("accum", 0, "dl_scaled", set()),
    "smooth_other_classes": ("smooth", 0, "dlogits", {"loss"}),
    "step2_momentum_init": ("b3", 1, "wire_sgd", {"momentum", "param"}),
    "stale_w2": ("b3", 1, "wire_conv2", {"wire_dgrad"}),
}


def test_every_planted_error_has_a_case():
    assert set(REJECT) == set(S.PLANTS)


@pytest.mark.parametrize("plant", S.PLANTS)
def test_checker_rejects_at_the_stage(plant):
    case, step, stage, also = REJECT[plant]
    good = S.check_step(S.emulate_case(case)[step])
    assert not S.failing(good), (plant, S.failing(good))
    res = S.check_step(S.emulate_case(case, plant)[step])
    bad = S.failing(res)
    assert bad and bad[0] == stage, (plant, [(s, res[s]) for s in bad])
    assert also <= set(bad), (plant, bad)
    if plant == "landing_shifted":
        assert res["landing"][1][0] in ("net.2.bias", "net.2.weight")  # the view it left, the view it hit
    if plant == "nominal_batch":  # the first, full batch of the same run is untouched
        assert not S.failing(S.check_step(S.emulate_case(case, plant)[0]))


def test_a_missing_or_extra_call_is_an_order_error():
    rec = dict(S.emulate_case("b1_bf16")[0])
    trace = rec["trace"]
    i = next(k for k, c in enumerate(trace) if c.name == "conv3x3_dgrad")
    res = S.check_step(dict(rec, trace=trace[:i] + trace[i + 1:]))
    assert S.failing(res) == ["order"] and "conv2 data gradient" in res["order"][1][0], res
    res = S.check_step(dict(rec, trace=trace[:-1] + [trace[3], trace[-1]]))
    assert S.failing(res) == ["order"] and "optimizer" in res["order"][1][0], res
    res = S.check_step(dict(rec, trace=trace + [trace[-1]]))
    assert S.failing(res) == ["order"] and "extra" in res["order"][1][0], res


def test_an_unwritten_element_is_out_of_bound():
    """What the recorder's NaN fill shows: one element a kernel did not write fails its stage."""
    rec = dict(S.emulate_case("b1_bf16")[0])
    trace = list(rec["trace"])
    c = trace[7]
    assert c.name == "conv3x3_wgrad"
    o = list(c.o)
    o[3] = o[3].clone()
    o[3][5, 18432 + 7] = float("nan")
    trace[7] = S.Call(c.name, c.a, o, c.kw, c.ko)
    res = S.check_step(dict(rec, trace=trace))
    assert S.failing(res)[0] == "w2slab" and res["w2slab"][0] == S.INF
    assert torch.isnan(trace[7].o[3]).sum() == 1
