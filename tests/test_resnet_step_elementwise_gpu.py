"""One ResNet-18 training step on the module path per element and stage against float64, on
MI355X: ops/resnet_fn.py's Functions, models/resnet.py forward_hip, ops/direct_grad.py and the
flat gradient space FusedSGD steps, recorded kernel call by kernel call and run through the
staged checker of tests/resnet_step_cases.py (whose docstring holds every bound;
tests/test_resnet_step_bounds_cpu.py shows the checker admitting a correct step and rejecting
thirteen planted wiring errors).  No production code changes for the recording: ``resnet_fn._C``,
``functional._C`` (the loss) and ``native.require`` (FusedSGD) are patched to a recording proxy.

Cases (the smallest shapes at which each path still exists):

  s64      64 x 64, batch 4, 10 classes (layer widths 16, 8, 4, 2), two consecutive steps: the first
           adds into the zeroed flat gradients and initialises momentum; the second runs after a
           lazy zero_grad with every gradient view pre-filled with NaN (it must overwrite),
           momentum in steady state, num_batches_tracked 2
  s72      72 x 72, batch 3, 1000 classes, label smoothing 0.1 (widths 18, 9, 5, 3): generic-width
           halo tiles, the halo weight gradient and its per-tap fallback, odd parity classes, the
           wave-per-row cross-entropy.  One step, after an unrecorded warm-up backward and a lazy
           zero_grad, gradient views NaN-filled (the first backward of a fresh model ADDS into the
           zeroed buffer - direct_grad.accumulate is True until a lazy zero_grad marks the
           parameters fresh - so NaN can only be pre-filled behind a lazy zero)
  accum    two micro-batches of 2 without zero_grad, one step: the second backward takes acc_w,
           acc_bn and the head's accumulating sgemm; reference = prior + sum (n + 1 terms)
  accum_ab after a lazy zero_grad, direct_grad.flush_fresh on the BatchNorm biases alone (the public
           path to "one of the pair fresh": beta's gradient zeroed and no longer fresh, gamma's
           fresh and NaN-filled): bn_bwd's ``ag != ab`` branch must clear dgamma and add both

s64 and s72 run on the materialised chain (resnet_fn.DEFER_BN False: every activation stored,
every stage checked) and on the default deferred chain, whose every stored tensor must equal the
materialised chain's bit for bit and whose trace must hold no bn_apply for a deferred BatchNorm
where the plan queries say conv2's halo forward and halo weight gradient apply it, and exactly
one materialising bn_apply where they do not.  (At these batch sizes the planner's automatic
halo forward, which wants a grid of 384 blocks, is never chosen: every conv2 materialises its
input and the stem's BatchNorm is the one applied by its consumer, the max pool.  The halo-applied
conv2 path stays with test_resnet_gpu.py's test_halo_conv_reads_deferred_batchnorm_bitwise.)
Run with -s for the RESNET_STEP_RATIO lines (profiles/resnet_step/README.md records them).

bn_finalize per element (stand-alone): ``resnet_step_cases.bn_finalize_bounds``.
"""
import contextlib

import pytest
import torch

import resnet_step_cases as S
from elementwise import BF, Guarded

pytestmark = pytest.mark.gpu
dev = "cuda"
_RESULTS = {}


@contextlib.contextmanager
def recording(C, defer):
    from ddp_amd import native
    from ddp_amd.ops import functional, resnet_fn

    rec = S.Recorder(C)
    saved = (resnet_fn._C, functional._C, native.require, resnet_fn.DEFER_BN)
    resnet_fn._C = functional._C = native.require = lambda: rec
    resnet_fn.DEFER_BN = bool(defer)
    try:
        yield rec
    finally:
        resnet_fn._C, functional._C, native.require, resnet_fn.DEFER_BN = saved


def build(cs):
    """The model with this file's parameters and BatchNorm buffers, its FusedSGD and loss."""
    from ddp_amd.models.resnet import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    model = resnet18(num_classes=cs["classes"])
    P, Bf = S.make_model(cs["classes"])
    with torch.no_grad():
        named = dict(model.named_parameters())
        assert list(named) == S.param_names()  # the case file's own description names the same parameters
        for n, v in P.items():
            assert named[n].shape == v.shape, n
            named[n].copy_(v)
        bufs = dict(model.named_buffers())
        for n, v in Bf.items():
            bufs[n].copy_(v)
    model = model.to(dev).train()
    opt = FusedSGD(model, **S.HP)
    fs = opt.flat
    lay = {n: (fs.offsets[n], fs.numels[n]) for n in fs.names}
    want, total = S.flat_layout({n: tuple(v.shape) for n, v in P.items()})
    assert lay == want and fs.numel == total
    return model, opt, CrossEntropyLoss(cs["label_smoothing"]), lay


def masters(model):
    return {n: p.detach().cpu().clone() for n, p in model.named_parameters()}


def poison(opt, skip=()):
    """NaN into every gradient view (not the alignment gaps) behind a lazy zero_grad."""
    from ddp_amd.ops import direct_grad

    for n in opt.flat.names:
        p = opt.flat.param(n)
        if n in skip:
            continue
        assert p in direct_grad._fresh, f"{n} is not fresh: NaN would be added to, not overwritten"
        opt.flat.view(opt.flat.grads, n).fill_(float("nan"))


def run_chain(C, case, defer):
    """[(trace, ctx, backwards)] per optimizer step of ``case`` on one chain."""
    cs = S.CASES["accum" if case == "accum_ab" else case]
    model, opt, lossf, lay = build(cs)
    out, nbt = [], 0
    batch = lambda seed: tuple(t.to(dev) for t in S.make_batch(cs["B"], cs["size"], cs["classes"], seed=seed))  # noqa: E731
    warm = case in ("s72", "accum_ab")
    if warm:  # an unrecorded backward, so that zero_grad is lazy and NaN can be pre-filled
        img, labels = batch(99)
        lossf(model(img), labels).backward()
        nbt += 1
    for step in range(cs["steps"]):
        micro = 1 if case == "accum_ab" else cs.get("micro", 1)
        if step or warm:
            from ddp_amd.ops import direct_grad

            opt.zero_grad()
            skip = ()
            if case == "accum_ab":
                skip = tuple(c["bn"] + ".bias" for c in S.TOPO["convs"])
                direct_grad.flush_fresh(opt.flat.param(n) for n in skip)
            poison(opt, skip)
        before = masters(model)
        grads_before = opt.flat.grads.detach().cpu().clone()
        with recording(C, defer) as rec:
            prior = None
            for mb in range(micro):
                img, labels = batch(10 * step + mb)
                if mb == micro - 1 and mb > 0:
                    torch.cuda.synchronize()
                    prior = {n: opt.flat.view(opt.flat.grads, n).detach().cpu().clone() for n in opt.flat.names}
                lossf(model(img), labels).backward()
                nbt += 1
            opt.step()
            torch.cuda.synchronize()
        ctx = dict(params=before, image=img.cpu(), labels=labels.cpu(), label_smoothing=cs["label_smoothing"],
                   nbt=nbt - 1, prior=prior, layout=lay, hp=S.HP, first_step=step == 0, grads_before=grads_before)
        out.append((rec.trace, ctx, micro))
    return out


def plan_materialise(C, st):
    """{conv2: does its deferred input get materialised} from the plan queries, at the shapes
    the materialised chain ran (resnet_fn._ConvBNAct.forward's rule)."""
    out = {}
    for c in S.TOPO["convs"]:
        if c["role"] != "conv2":
            continue
        f = st["fwd"][c["name"]]["conv"]
        x, y = torch.empty(f.a[0].shape, dtype=BF, device=dev), torch.empty(f.o[3].shape, dtype=BF, device=dev)
        halo = C.conv_gemm_plan(x, y, 3, 3, 1, 1)[5]
        ppc = C.conv_gemm_wgrad_ppc(x, y, 3, 3, 1, 1)
        out[c["name"]] = not (halo == 1 and C.conv_gemm_wgrad_uses_halo(x, y, 3, 3, 1, 1, ppc))
    return out


def results(C, case):
    """{"stages": [res per step], "chains": [(names compared, names that differ, materialise)]}
    of a case, computed once."""
    if case in _RESULTS:
        return _RESULTS[case]
    out = dict(stages=[], chains=[], flags=[])
    mat = run_chain(C, case, defer=False)
    parsed = []
    for k, (trace, ctx, backwards) in enumerate(mat):
        res = S.check_step(trace, ctx, backwards)
        S.report(res, f"{case}_step{k}" if len(mat) > 1 else case)
        out["stages"].append(res)
        parsed.append(S.parse_trace(trace, backwards) if "order" not in S.failing(res) else None)
        if parsed[-1] is not None:
            st = parsed[-1][0][-1]
            flags = {c.a[12] for c in st["head_bwd"][1:]}
            for bw in st["bwd"].values():
                flags |= {bw["bn"].a[11], bw["red"].a[0][0][7] if bw["red"] is not None else bw["wgrad"].a[8]}
            out["flags"].append(([n for n, bw in st["bwd"].items() if bw["red"] is not None], flags))
    if case in ("s64", "s72") and all(p is not None for p in parsed):
        dfr = run_chain(C, case, defer=True)
        for (sts, sgd), (trace, ctx, backwards) in zip(parsed, dfr):
            m = plan_materialise(C, sts[-1])
            try:
                dsts, dsgd = S.parse_trace(trace, backwards, materialise=m)
            except S.OrderError as e:
                out["chains"].append((0, [str(e)], m))
                continue
            a, b = S.stored(sts[-1]), S.stored(dsts[-1])
            a.update(params=sgd.o[0], momentum=sgd.o[2], grads=sgd.a[1])
            b.update(params=dsgd.o[0], momentum=dsgd.o[2], grads=dsgd.a[1])
            extra = sorted(set(b) - set(a))
            diff = [n for n in b if n in a and S.bitwise(b[n], a[n])[0] != 0.0]
            out["chains"].append((len(b), extra + diff, m))
    _RESULTS[case] = out
    return out


@pytest.mark.parametrize("case", ["s64", "s72", "accum", "accum_ab"])
def test_every_stage_within_its_bound(C, case):
    r = results(C, case)
    assert len(r["stages"]) == S.CASES["accum" if case == "accum_ab" else case]["steps"]
    for k, res in enumerate(r["stages"]):
        bad = S.failing(res)
        assert not bad, f"{case} step {k}: out of bound at {[(s, res[s]) for s in bad]}"
        assert set(res) == set(S.STAGES), set(S.STAGES) ^ set(res)  # every stage ran, every output finite


@pytest.mark.parametrize("case", ["s64", "s72"])
def test_deferred_chain_equals_materialised_chain(C, case):
    r = results(C, case)
    assert len(r["chains"]) == len(r["stages"])
    for n, diff, m in r["chains"]:
        print(f"RESNET_STEP_CHAINS {case} compared {n} materialised {sorted(k for k, v in m.items() if v)}")
        assert not diff, f"{case}: the deferred chain differs at {diff}"
        assert n > 200
    if case == "s72":  # layer4's 3 x 3 images: the halo weight gradient's gate refuses them
        m = r["chains"][0][2]
        assert m["layer4.0.conv2"] and m["layer4.1.conv2"], m


def test_cases_reach_both_weight_gradient_paths_and_every_accumulate_flag(C):
    """s64 takes the slab + grad_reduce path somewhere and the one-chunk path elsewhere.  The first
    backward of a fresh model and accum's second backward pass accum = True to every producer;
    s64's second step (behind a lazy zero_grad) passes False to every one."""
    for case, step, want in (("s64", 0, True), ("s64", 1, False), ("accum", 0, True)):
        reds, flags = results(C, case)["flags"][step]
        assert flags == {want}, (case, step, flags)
        if case == "s64":
            assert reds and len(reds) < 20, reds


# ------------------------------------------------------------------- bn_finalize per element
# (rows, C, count)
FIN_CASES = [(1, 64, 1), (1, 512, 16), (1, 96, 50), (7, 96, 896), (130, 64, 1040), (200, 512, 1600), (65, 96, 65)]


@pytest.mark.parametrize("rows,Cc,count", FIN_CASES)
def test_bn_finalize_per_element(C, rows, Cc, count):
    """mean, invstd, running_mean, running_var per element against float64 of the same slab.
    Channel 0: mean 8, deviation 2**-6 (the worst cancellation: the bound widens, see the CPU
    file); channel 1: a constant (the clamp: invstd = rsqrt(eps) within bound)."""
    G = C.bn_finalize_groups(rows)
    assert (G > 1) == (rows > 64)
    g = torch.Generator().manual_seed(rows * 1000 + Cc + count)
    per = max(count // rows, 1)
    assert per * rows == count
    x = torch.randn(rows, per, Cc, generator=g, dtype=torch.float64) * (torch.rand(Cc, generator=g, dtype=torch.float64) * 2 + 0.1) \
        + torch.randn(Cc, generator=g, dtype=torch.float64)
    sign = (1 - 2 * (torch.arange(rows * per) % 2)).double().view(rows, per)
    x[..., 0] = 8.0 + 2.0 ** -6 * sign
    x[..., 1] = 1.7
    slab = torch.stack([x.sum(1), (x * x).sum(1)], 1).float().to(dev)  # [rows][2][C]
    rm0 = torch.randn(Cc, generator=g).to(dev)
    rv0 = (torch.rand(Cc, generator=g) + 0.5).to(dev)
    bufs = [Guarded(Cc, torch.float32, guard=1024) for _ in range(4)]
    rm, rv, mean, invstd = (b.t for b in bufs)
    rm.copy_(rm0)
    rv.copy_(rv0)
    nbt = torch.tensor(5, device=dev)
    ws = torch.full((G, 2, Cc), float("nan"), device=dev)
    C.bn_finalize(slab, rows, Cc, float(count), 1e-5, 0.1, rm, rv, mean, invstd, nbt, ws)
    torch.cuda.synchronize()
    b = S.bn_finalize_bounds(slab, count, 1e-5, 0.1, rm0, rv0)
    for k, t in (("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rv)):
        r, i = S.worst(t, *b[k])
        print(f"RESNET_STEP_RATIO bn_finalize_{(rows, Cc, count)} {k} {r:.3e}")
        assert r <= 1.0, f"bn_finalize {(rows, Cc, count)} {k}: error / bound = {r:.3f} at channel {i}"
    assert int(nbt) == 6
    for b_ in bufs:
        b_.check("C channels")
    # the bound itself says where fp32 runs out: the cancelling channel is allowed parts per thousand or more
    ref, bound = b["invstd"]
    if count > 1:
        assert 1e-3 < bound[0] / ref[0]
    assert abs(ref[1].item() - 1e-5 ** -0.5) / 1e-5 ** -0.5 < 0.05  # the constant channel: rsqrt(eps)
