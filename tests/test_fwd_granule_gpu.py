"""The level-3 forward's cross-block hand-off: partial logits published as tagged 8-byte
granules {tag, float bits} and swept by wave 0 of every block of the image (launchers.h
FwdDz, conv3x3_fwd_body.inc.h).

Every comparison is bitwise: the level-3 engine against the level-1 engine from the same seed
(the level-1 chain sums the same partials in the fc backward's prologue, with no in-launch
hand-off at all), parameters and the loss history after the run.  A sweep that accepted a
granule of an earlier step or epoch, or read a torn / stale one, would change a logit and with
it every later parameter.  No test provokes the bounded wait's timeout."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"


def _mk(n, B, level, dtype="bf16", use_graph=True, graph_steps=2, momentum=0.9, pxt_fwd=None, seed=0):
    from ddp_amd.data import DeviceMNIST, synthetic_mnist
    from ddp_amd.engine import EngineOptions, FusedSimpleCNNEngine
    from ddp_amd.models import SimpleCNN
    from ddp_amd.ops import FusedSGD

    torch.manual_seed(seed)
    model = SimpleCNN(compute_dtype=torch.float32 if dtype == "fp32" else torch.bfloat16).to(dev)
    opt = FusedSGD(model, lr=0.01, momentum=momentum, weight_decay=1e-4)
    imgs, labels = synthetic_mnist(n)
    eng = FusedSimpleCNNEngine(model, opt, DeviceMNIST(imgs, labels, dev), B, 1, 0,
                               opts=EngineOptions(graph_steps=graph_steps, use_graph=use_graph, fuse_level=level,
                                                  dtype=dtype, pxt_fwd=pxt_fwd, store_a1=0))
    eng.refresh()
    return model, opt, eng


def _same(m1, o1, e1, m3, o3, e3):
    assert e3.level3 and e3.eng.last_level3 and not e1.level3
    assert e3.eng.sync_error == 0 and e1.eng.sync_error == 0
    for (k, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
        assert torch.equal(a, b), k
    if o1.momentum_buffer is not None:
        assert torch.equal(o1.momentum_buffer, o3.momentum_buffer)
    assert torch.equal(e1.t["loss_hist"], e3.t["loss_hist"])
    assert torch.equal(e1.t["step_ctr"], e3.t["step_ctr"])
    assert torch.isfinite(e3.fs.params).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("pxt", [1, 2])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_granule_handoff_geometry(B, pxt, dtype):
    """B = 1: the last block is cut by the pixel count (784 / 64 = 12.25 blocks).  B >= 2: blocks
    that straddle two images publish and sweep slot 1, and an image's first block index times
    the block size is not its first pixel.  B = 5 at pxt 2: an image whose first and last blocks
    are both shared.  6 steps: the eager momentum step, two 2-step graph replays, one eager."""
    runs = []
    for level in (1, 3):  # one engine at a time: the level-3 forward needs its whole grid resident
        m, o, e = _mk(64, B, level, dtype=dtype, pxt_fwd=pxt)
        e.run_steps(6)
        e.synchronize()
        runs += [m, o, e]
    _same(*runs)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("n", [4, 7, 11])
def test_granule_tags_never_go_stale(n, use_graph):
    """B = 4 for 4 epochs.  n = 4: one-step epochs - the step counter restarts every step, so a
    tag derived from it would recur and last epoch's granules would satisfy the sweep.  n = 7:
    a full step plus a ragged one of 3 images (fewer blocks: the full step's granules of the
    higher blocks stay behind).  n = 11: two full steps (one 2-step graph replay when graphed;
    at n = 4 and 7 an epoch has no full replay and every step runs eagerly) plus the ragged
    step.  A granule left by an earlier step or epoch must never satisfy a later sweep."""
    runs = []
    for level in (1, 3):
        m, o, e = _mk(n, 4, level, use_graph=use_graph, graph_steps=2)
        for ep in range(4):
            e.run_epoch(ep)
        e.synchronize()
        if level == 3:
            assert e.eng.level3_active(4) and (n % 4 == 0 or e.eng.level3_active(n % 4))
        runs += [m, o, e]
    _same(*runs)


def test_granule_handoff_under_uneven_load():
    """B = 8, 200 graph-replayed steps while a side stream streams large elementwise copies
    through the GPU for the duration (blocks of an image reach their hand-off far apart, the
    sweeps compete with the copies' traffic); the result equals the unloaded level-1 run."""
    m1, o1, e1 = _mk(2048, 8, 1, graph_steps=50)
    e1.run_steps(201)  # (the eager momentum step + 4 replays)
    e1.synchronize()
    m3, o3, e3 = _mk(2048, 8, 3, graph_steps=50)
    side = torch.cuda.Stream()
    src = torch.rand(32 << 20, device=dev)  # 128 MB
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    done = 0
    while done < 201:
        with torch.cuda.stream(side):
            for _ in range(24):
                dst.copy_(src)
        done += e3.run_steps(51 if done == 0 else 50)
    busy = not side.query()  # the copies outlast the steps' launch
    e3.synchronize()
    side.synchronize()
    print(f"side stream still busy after the last replay was enqueued: {busy}")
    _same(m1, o1, e1, m3, o3, e3)
