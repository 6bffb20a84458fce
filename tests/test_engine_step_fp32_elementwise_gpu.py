"""One exact-fp32 step of the fused SimpleCNN engine (``--dtype fp32``, engine.cpp
launch_step_t<float>), stage by stage and element by element against float64, on MI355X.  The
sibling of tests/test_engine_step_elementwise_gpu.py for the fp32 table of
tests/engine_step_cases.py (``prec="fp32"``: every bound 3 n u A, no bf16 term; shown to admit
and reject by tests/test_engine_step_bounds_cpu.py).

Reached here and by no stand-alone binding: the conv backward with both roles split over
input-channel halves at two blocks per CU (wgrad_split = 2), the dgrad role reading w2t_f32 from
global memory, the conv1 recompute in place of a stored a1, the fp32 dZ2 and fc role of the
level-3 chain, the w2t_f32 / wfc_frag32 copies a real previous step left, and the slab reduction
in its own grad_reduce launch (the fp32 default) or fused - the four reduced gradients must be,
bit for bit, the float32 replay of slab_reduce.h's order over the stored slab rows on both.

Before the checked step a2, dz2, fc_part, dlogits, loss_rows, both slabs and the flat gradient
views are filled with NaN: a stage the chain should have written and did not is non-finite, and
on a ragged batch the rows past B must still be NaN.  One engine at a time (level 3's forward
spins on the other blocks of its images); only chain / batch / option combinations
tests/test_fp32_gpu.py already launches.

Run with -s for the STEP_RATIO fp32_<chain> <B> <stage> <error / bound> lines;
profiles/engine_step/README.md records them.
"""
import functools

import pytest
import torch

import engine_step_harness as H
from engine_step_harness import begin

pytestmark = pytest.mark.gpu
L1 = dict(fuse_level=1, wgrad_split=1)  # the round-3 kernels: one conv backward block per row / chunk
L3 = dict(fuse_level=3, wgrad_split=2, momentum=0.9, weight_decay=1e-4)
# the fp32 description: dtype="fp32" fixed, the chain left to the engine's defaults unless a test names it
_setup = functools.partial(H.setup, H.FP32)
checked_step = functools.partial(H.checked_step, H.FP32)


# ------------------------------------------------------------------------------- level 1
@pytest.mark.parametrize("B", [1, 12, 32, 64])
def test_level1_first_step(B):
    """The round-3 kernels (one conv backward block per slab row and pixel chunk, dL in fc_bwd's
    prologue), every gradient in the flat buffer, then sgd_kernel: R = 1 (28 rows), 2 (168), 4
    (224, 448)."""
    eng, imgs, labels = _setup(B=B, fuse_opt=False, **L1)
    assert not eng.level3
    begin(eng)
    res = checked_step(eng, imgs, labels, B, "l1", first_step=True)
    assert "fc_part" in res and "grad_wfc" in res and "dlogits" not in res


# ------------------------------------------------------------------------------- level 3
@pytest.mark.parametrize("B,role,fred,fuse_opt", [(1, 1, None, True), (20, 1, None, True), (32, 1, None, True),
                                                  (40, 1, None, True), (32, 0, None, True), (32, 1, 1, True),
                                                  (32, 1, None, False), (32, 1, 1, False)])
def test_level3_first_step(B, role, fred, fuse_opt):
    """dL and dZ2 in the forward, both conv backward roles split over channel halves, the fc
    weight gradient as a role (1) or its own kernel (0), the slab reduction in grad_reduce (fred
    None, the fp32 default) or fused into the conv backward (1); fuse_opt False keeps the fc
    weight gradient in the flat buffer too."""
    eng, imgs, labels = _setup(B=B, l3_fc_role=role, fuse_reduce=fred, fuse_opt=fuse_opt, **L3)
    assert eng.level3
    begin(eng)
    chain = "l3" + ("" if role else "_fckernel") + ("_fred" if fred else "") + ("" if fuse_opt else "_sgd")
    res = checked_step(eng, imgs, labels, B, chain, first_step=True)
    assert eng.eng.last_level3 and eng.eng.last_fc_role == (role > 0)
    if B == 32:  # 224 + 196 rows: the 16-group order, and the fused reducers fit
        assert eng.eng.last_fused_reduce == (fred == 1)
    assert ("grad_wfc" in res) == (not fuse_opt) and "momentum_w2" in res


def test_level3_fourth_step():
    """Three real steps, then the fourth checked: the w2t_f32 and wfc_frag32 the third step's
    SGD left, the steady-state momentum rule, loss_hist[3], the index window [96, 128)."""
    eng, imgs, labels = _setup(B=32, **L3)
    begin(eng)
    for _ in range(3):
        eng.eng.step(32, 32)
    res = checked_step(eng, imgs, labels, 32, "l3_step3")
    assert eng.t["step_ctr"].item() == 4 and "momentum_w2" in res


def test_level3_ragged_tail_then_next_epoch():
    """n = 100 at B = 32: three full steps, the 4-image tail at its real size (1 / 4, its 28 + 25
    slab rows - the 4-group order - among the full batch's, the rows past it untouched), then the
    first step of epoch 1 on the reshuffled index list."""
    eng, imgs, labels = _setup(n=100, B=32, **L3)
    begin(eng)
    for _ in range(3):
        eng.eng.step(32, 32)
    checked_step(eng, imgs, labels, 4, "l3_tail_of_32")
    assert eng.eng.level3_active(4) and eng.eng.last_level3 and eng.eng.last_fc_role
    first = eng.sampler.indices()[:32].clone()
    begin(eng, 1)  # the reshuffled index list, loss slot 0 again
    assert not torch.equal(eng.sampler.indices()[:32], first)
    checked_step(eng, imgs, labels, 32, "l3_epoch1")


def test_level3_eager_step_after_graph_replay():
    """The momentum-init step, five captured steps replayed, then one eager step checked."""
    eng, imgs, labels = _setup(B=32, use_graph=True, graph_steps=5, **L3)
    eng.run_steps(6)
    eng.synchronize()
    assert eng._captured == 5 and eng.t["step_ctr"].item() == 6
    checked_step(eng, imgs, labels, 32, "l3_after_replay")


def test_defaults_resolve_to_level3_fc_role_and_the_separate_reduction():
    """EngineOptions(dtype="fp32") with nothing else set."""
    eng, imgs, labels = _setup(B=32)
    assert eng.level3 and eng.cfg["fuse_level"] == 3 and eng.cfg["wgrad_split"] == 2 and eng.cfg["fuse_reduce"] == 0
    begin(eng)
    checked_step(eng, imgs, labels, 32, "default", first_step=True)
    assert eng.eng.last_level3 and eng.eng.last_fc_role and not eng.eng.last_fused_reduce
