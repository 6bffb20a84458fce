"""One SimpleCNN training step on the module path per element and stage against float64, on MI355X:
ops/functional.py's four autograd Functions, SimpleCNN.forward, the FlatSpace gradient views,
DistributedDataParallel's hooks and FusedSGD, recorded kernel call by kernel call and run through
the staged checker of tests/simplecnn_step_cases.py (whose docstring holds every stage, bound and
wiring assertion; tests/test_simplecnn_step_bounds_cpu.py shows the checker admitting a correct
step and rejecting fourteen planted wiring errors).  No production code changes for the
recording: ``functional._C`` and ``native.require`` (FusedSGD) are patched to a recording proxy
that fills every output argument with NaN before the launch; tensor hooks on the parameters keep
the gradients the Functions return.

Cases (28 x 28 x (1 -> 32 -> 64), 10 classes are fixed: the batch is the only free shape):

  b1         one image, bf16 and fp32: 784 pixels leave the last forward / dgrad block partly filled
  b3         bf16, blocks straddle images; two consecutive steps, momentum 0.9, weight decay 5e-4:
             the momentum-init step and the steady state.  SimpleCNN's module path takes no lazy
             zero (AccumulateGrad adds into the views): the views are zero before the backward
             (``zeroed``) and prior + new holds (``landing``); step 2 reads step 1's masters
  b10, b19   bf16 and fp32, and b32 bf16: the remaining wgrad_rows branches (R = 2, 4, 7), odd B
  ragged     DeviceMNISTLoader over a 17-image DeviceMNIST, nominal batch 10: the steps of 10 and
             of 7 images (1 / 7), the loader's uint8 -> float hand-off
  smooth     b3 with CrossEntropyLoss(label_smoothing=0.1)
  accum      two micro-batches of 3 without zero_grad, loss / 2 as _run_module_epoch scales it, one sgd
  input_grad b1 fp32 with x.requires_grad_(): the conv_transpose2d fallback of _Conv1ReLU.backward
  ddp1       (no recording) b3 and accum under DistributedDataParallel at world size 1: bit for bit
             the bare model; allreduce_buckets_launched per synced backward, none under no_sync
  graphed    (no recording) b3 in GraphedStep(warmup=1) plus two replays: bit for bit three eager steps

Run with -s for the SIMPLECNN_STEP_RATIO lines (profiles/simplecnn_step/README.md records them).
"""
import contextlib

import pytest
import torch

import simplecnn_step_cases as S

pytestmark = pytest.mark.gpu
dev = "cuda"
_RESULTS = {}


@contextlib.contextmanager
def recording(C):
    from ddp_amd import native
    from ddp_amd.ops import functional

    rec = S.Recorder(C, S.KERNELS, S.OUTPUTS)
    saved = (functional._C, native.require)
    functional._C = native.require = lambda: rec
    try:
        yield rec
    finally:
        functional._C, native.require = saved


def build(cs):
    """The model with the case file's masters, its FusedSGD and loss."""
    from ddp_amd.models import SimpleCNN
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    model = SimpleCNN(compute_dtype=cs["dtype"])
    with torch.no_grad():
        named = dict(model.named_parameters())
        assert tuple(named) == S.NAMES
        for n, v in S.masters().items():
            assert tuple(named[n].shape) == S.SHAPES[n], n
            named[n].copy_(v)
    model = model.to(dev).train()
    opt = FusedSGD(model, **S.HP)
    return model, opt, CrossEntropyLoss(cs["eps"])


def batches(case):
    """Per optimizer step, per pass: (x on the device, u8 on the CPU or None, labels on the device)."""
    cs = S.CASES[case]
    if not cs["loader"]:
        return [[(x.to(dev), None, y.to(dev)) for x, _, y in passes] for passes in S.case_inputs(case)]
    from ddp_amd.data.loader import DeviceMNIST, DeviceMNISTLoader

    u8, labels = S.loader_dataset()
    loader = DeviceMNISTLoader(DeviceMNIST(u8, labels, dev), 10, 1, 0)
    idx = loader.sampler.indices().cpu().long()
    out = [[(x, u8[idx[10 * k:10 * k + 10]], y)] for k, (x, y) in enumerate(loader)]
    assert [p[0][0].shape[0] for p in out] == [10, 7] and len(loader) == 2
    for (x, u, y), in out:
        assert torch.equal(y.cpu(), labels[idx][:10] if x.shape[0] == 10 else labels[idx][10:])
    return out


def run_case(C, case):
    """[step record] of ``case``, as simplecnn_step_cases.check_step reads it."""
    cs = S.CASES[case]
    model, opt, lossf = build(cs)
    fs = opt.flat
    lay = {n: (fs.offsets[n], fs.numels[n]) for n in fs.names}
    hooked = {}
    for n, p in model.named_parameters():
        p.register_hook(lambda g, n=n: hooked.__setitem__(n, g.detach().clone()))
    out = []
    for si, passes in enumerate(batches(case)):
        opt.zero_grad()
        torch.cuda.synchronize()
        before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        mom = None if opt.momentum_buffer is None else opt.momentum_buffer.cpu().clone()
        micro = []
        with recording(C) as rec:
            for x, u8, y in passes:
                gb = fs.grads.cpu().clone()
                hooked.clear()
                if cs["input_grad"]:
                    x = x.clone().requires_grad_()
                loss = lossf(model(x), y)
                (loss / cs["accum"] if cs["accum"] > 1 else loss).backward()
                torch.cuda.synchronize()
                micro.append(dict(x=x.detach().cpu(), u8=u8, labels=y.cpu(), scale=1.0 / cs["accum"], eps=cs["eps"],
                                  hooked={n: g.cpu() for n, g in hooked.items()}, grads_before=gb,
                                  grads_after=fs.grads.cpu().clone(), gx=x.grad.cpu() if cs["input_grad"] else None))
            opt.step()
            torch.cuda.synchronize()
        out.append(dict(trace=rec.trace, params=before, momentum_before=mom, first_step=si == 0, dtype=cs["dtype"],
                        layout=lay, total=fs.numel, hp=S.HP, micro=micro))
    return out


def results(C, case):
    if case not in _RESULTS:
        recs = run_case(C, case)
        res = [S.check_step(r) for r in recs]
        for k, r in enumerate(res):
            S.report(r, f"{case}_step{k}" if len(res) > 1 else case)
        _RESULTS[case] = (recs, res)
    return _RESULTS[case]


@pytest.mark.parametrize("case", list(S.CASES))
def test_every_stage_within_its_bound(C, case):
    cs = S.CASES[case]
    recs, res = results(C, case)
    assert len(res) == len(cs["steps"])
    want = set(S.STAGES) - (set() if cs["input_grad"] else {"input_grad"})
    for k, r in enumerate(res):
        bad = S.failing(r)
        assert not bad, f"{case} step {k}: out of bound at {[(s, r[s]) for s in bad]}"
        assert set(r) == want, want ^ set(r)  # every stage ran, every output finite
    for rec, sizes in zip(recs, cs["steps"]):  # the slabs are sized with the extension's own block counts
        sts, _ = S.parse_trace(rec["trace"], len(sizes))
        for st, B in zip(sts, sizes):
            Rr = S.wgrad_rows(28, B, cs["dtype"])
            assert Rr == S.WGRAD_ROWS.get((cs["dtype"], B), Rr)
            assert st["wg"].o[3].shape[0] == C.conv3x3_wgrad_blocks(B, 28, Rr)
            assert st["c1w"].o[7].shape[0] == C.conv1_wgrad_blocks(B, 28, 28, 256)
            assert st["xe"].a[8] == 1.0 / B


def test_second_step_reads_the_first_steps_masters(C):
    """b3's step 2: the masters the checker held conv2's operands to are step 1's output, and differ
    from the initial ones in the bf16 operand itself."""
    recs, _ = results(C, "b3")
    sgd0 = recs[0]["trace"][-1]
    assert S.bitwise(S.to_flat(recs[1]["params"], recs[1]["layout"], recs[1]["total"]), sgd0.o[0])[0] == 0.0
    w0, w1 = recs[0]["trace"][1].a[1], recs[1]["trace"][1].a[1]
    assert w0.dtype == torch.bfloat16 and bool((w0 != w1).any())
    assert recs[1]["first_step"] is False and S.bitwise(recs[1]["momentum_before"], sgd0.o[2])[0] == 0.0


def run_plain(case, steps=None, wrap=None, counts=None):
    """``case`` without recording: (flat gradients, parameters, momentum) after its steps.  ``wrap``:
    model -> DistributedDataParallel; ``counts`` then receives allreduce_buckets_launched after every
    backward."""
    cs = S.CASES[case]
    model, opt, lossf = build(cs)
    net = wrap(model) if wrap is not None else model
    for passes in (steps if steps is not None else batches(case)):
        opt.zero_grad()
        for k, (x, _, y) in enumerate(passes):
            loss = lossf(net(x), y)
            loss = loss / cs["accum"] if cs["accum"] > 1 else loss
            sync = k == len(passes) - 1 or wrap is None
            with contextlib.nullcontext() if sync else net.no_sync():
                loss.backward()
            if counts is not None:
                counts.append(net.allreduce_buckets_launched)
        opt.step()
    torch.cuda.synchronize()
    return opt.flat.grads.cpu(), opt.flat.params.cpu(), opt.momentum_buffer.cpu()


def test_ddp_world1_is_the_bare_model_bit_for_bit(C):
    import torch.distributed as dist

    from ddp_amd.parallel import DistributedDataParallel

    bare = {case: run_plain(case) for case in ("b3", "accum")}
    recs, _ = results(C, "b3")  # recording (the NaN fill, the hooks) changes nothing either
    assert S.bitwise(bare["b3"][1], recs[1]["trace"][-1].o[0])[0] == 0.0
    dist.init_process_group("nccl", rank=0, world_size=1, store=dist.HashStore(), device_id=torch.device("cuda", 0))
    try:
        made = []

        def wrap(model):
            made.append(DistributedDataParallel(model))
            return made[-1]

        for case in ("b3", "accum"):
            counts = []
            got = run_plain(case, wrap=wrap, counts=counts)
            for name, a, b in zip(("grads", "params", "momentum"), got, bare[case]):
                assert S.bitwise(a, b)[0] == 0.0, f"{case}: {name} differ under DistributedDataParallel"
            nb = len(made[-1].buckets)
            assert nb == 2
            assert counts == ([nb, 2 * nb] if case == "b3" else [0, nb]), (case, counts)
    finally:
        dist.destroy_process_group()


def test_graphed_step_is_three_eager_steps_bit_for_bit(C):
    from ddp_amd.engine import GraphedStep

    g = torch.Generator().manual_seed(77)
    data = [(torch.rand(3, 1, 28, 28, generator=g).to(dev), None, torch.randint(0, 10, (3,), generator=g).to(dev))
            for _ in range(3)]
    eager = run_plain("b3", steps=[[d] for d in data])
    model, opt, lossf = build(S.CASES["b3"])

    def step(x, y):
        opt.zero_grad()
        loss = lossf(model(x), y)
        loss.backward()
        opt.step()
        return loss

    gs = GraphedStep(step, (data[0][0], data[0][2]), warmup=1)
    for x, _, y in data[1:]:
        gs(x, y)
    torch.cuda.synchronize()
    assert gs.replays == 2
    for name, a, b in zip(("grads", "params", "momentum"), (opt.flat.grads, opt.flat.params, opt.momentum_buffer), eager):
        assert S.bitwise(a.cpu(), b)[0] == 0.0, f"{name} differ between the captured and the eager steps"
