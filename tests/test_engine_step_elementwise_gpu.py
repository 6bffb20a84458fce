"""One bf16 step of the fused SimpleCNN engine, stage by stage and element by element against
float64, on MI355X.

tests/test_simplecnn_kernels_elementwise_gpu.py holds each kernel against float64 with its own
buffers and arguments at B = 1 and 3; the engine tests pin the chains to each other bit for bit
and to a whole-tensor 1e-2 norm at one batch size.  This file holds what engine.cpp
launch_step_t wires together at the batch sizes the engine runs: every buffer of ``eng.t`` a
step materialises goes through tests/engine_step_cases.py ``check_step`` (teacher-forced float64
references, a-priori bounds of ddp_amd/ops/kernel_bounds.py - derived in that module's
docstring, shown to admit and reject by tests/test_engine_step_bounds_cpu.py).  Seen here and
nowhere else per element: the batch the step gathers (index list x step counter, ragged tail,
reshuffled epoch), 1 / B of a ragged batch, the slab rows wgrad_rows(28, B) implies and the
reducer's row count, the pxt 1 / pxt 2 and OCC-2 forward by batch, the shadows a real previous
step (eager or replayed) left, loss_hist[step], the offsets of the flat gradient buffer.

Before the checked step a1, a2, dz1, dz2, fc_part, dlogits, loss_rows, both slabs and the flat
gradient buffer are filled with NaN: a stage the chain should have written and did not is
non-finite (infinitely out of bound), and on a ragged batch the rows past B must still be NaN.

Run with -s for the STEP_RATIO <chain> <B> <stage> <error / bound> lines;
profiles/engine_step/README.md records them.
"""
import functools

import pytest
import torch

import engine_step_harness as H
from engine_step_harness import begin

pytestmark = pytest.mark.gpu
# the bf16 description: a1 stored for the mask (store_a1 = 1), the level-0 chain unless a test says otherwise
_setup = functools.partial(H.setup, H.BF16)
checked_step = functools.partial(H.checked_step, H.BF16)


# ------------------------------------------------------------------------------- level 0
@pytest.mark.parametrize("fuse_opt", [False, True], ids=["sgd_kernel", "fused_opt"])
@pytest.mark.parametrize("B", [1, 3, 20, 32, 33, 64])
def test_level0_first_step(B, fuse_opt):
    """The 8-kernel chain (no in-launch waits) at every batch size that takes another path:
    B = 1, 3 (R = 1: 28 and 84 slab rows), 20 (R = 4: 140 rows), 32 (R = 7: 128 rows), 33 (an odd
    count past 32: 132 rows, 25872 pixels - no multiple of the forward's or the data gradient's
    block), 64 (the pxt-2 forward, 256 rows).  fuse_opt False: every gradient
    in the flat buffer, then the flat SGD kernel; True: the optimizer in the epilogues, with
    momentum and weight decay."""
    kw = dict(momentum=0.9, weight_decay=1e-4) if fuse_opt else {}
    eng, imgs, labels = _setup(B=B, fuse_level=0, fuse_opt=fuse_opt, **kw)
    begin(eng)
    res = checked_step(eng, imgs, labels, B, f"l0_{'fopt' if fuse_opt else 'sgd'}", first_step=fuse_opt)
    assert ("grad_wfc" in res) == (not fuse_opt)


# ------------------------------------------------------------------------- levels 1 and 3
@pytest.mark.parametrize("level,B,role", [(1, 1, 1), (1, 20, 1), (1, 32, 1), (1, 40, 1), (1, 64, 1),
                                          (3, 1, 1), (3, 20, 1), (3, 32, 1), (3, 40, 1), (3, 64, 1), (3, 32, 0)])
def test_fused_levels_first_step(level, B, role):
    """The 3-kernel and the 2-kernel chain at batch sizes the suite already launches on them,
    a1 stored for the mask, the fc weight gradient as a role of the conv backward and as its own
    kernel.  One engine at a time (tests/test_engine_gpu.py: level 3's forward spins on the
    other blocks of its images)."""
    eng, imgs, labels = _setup(B=B, fuse_level=level, momentum=0.9, weight_decay=1e-4, l3_fc_role=role)
    assert eng.level3 == (level == 3)
    begin(eng)
    checked_step(eng, imgs, labels, B, f"l{level}" + ("" if role else "_fckernel"), first_step=True)
    if level == 3:
        assert eng.eng.last_level3 and eng.eng.last_fc_role == (role > 0)


# -------------------------------------------------------------------------------- step k > 0
@pytest.mark.parametrize("level", [0, 3])
def test_fourth_step(level):
    """Three real steps, then the fourth checked: the shadows the third step's SGD left, the
    steady-state momentum rule, loss_hist[3], the index window [3 B, 4 B)."""
    eng, imgs, labels = _setup(B=32, fuse_level=level, momentum=0.9, weight_decay=1e-4)
    begin(eng)
    for _ in range(3):
        eng.eng.step(32, 32)
    res = checked_step(eng, imgs, labels, 32, f"l{level}_step3")
    assert eng.t["step_ctr"].item() == 4 and "momentum_w2" in res


# ------------------------------------------------------------------------------ ragged tail
def ragged(level, n, B):
    eng, imgs, labels = _setup(n=n, B=B, fuse_level=level, momentum=0.9, weight_decay=1e-4)
    nfull, rem = divmod(n, B)
    begin(eng)
    for _ in range(nfull):
        eng.eng.step(B, B)
    checked_step(eng, imgs, labels, rem, f"l{level}_tail_of_{B}")
    if level == 3:
        assert eng.eng.level3_active(rem) and eng.eng.last_level3 and eng.eng.last_fc_role
    first = eng.sampler.indices()[:B].clone()
    begin(eng, 1)  # the reshuffled index list, loss slot 0 again
    assert not torch.equal(eng.sampler.indices()[:B], first)
    checked_step(eng, imgs, labels, B, f"l{level}_epoch1")


@pytest.mark.parametrize("n,B", [(200, 64), (100, 32)])
def test_level0_ragged_tail_then_next_epoch(n, B):
    """The last step of an epoch at its real size (8 of 64, 4 of 32: 1 / B of the tail, its slab
    rows among the full batch's, the rows past it untouched), then the first step of epoch 1."""
    ragged(0, n, B)


def test_level3_ragged_tail_then_next_epoch():
    """The same on the 2-kernel chain at B = 64 / tail 8 (what test_fuse_level3_ragged_epoch runs)."""
    ragged(3, 200, 64)


# ------------------------------------------------------------------------ after graph replay
def test_level3_eager_step_after_graph_replay():
    """The momentum-init step, five captured steps replayed, then one eager step checked: the
    state a replay leaves (shadows, step counter, granule generation) is what a step expects."""
    eng, imgs, labels = _setup(B=32, fuse_level=3, momentum=0.9, weight_decay=1e-4, use_graph=True, graph_steps=5)
    eng.run_steps(6)
    eng.synchronize()
    assert eng._captured == 5 and eng.t["step_ctr"].item() == 6
    checked_step(eng, imgs, labels, 32, "l3_after_replay")
