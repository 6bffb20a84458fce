"""image_gather_mix_nhwc4 and the PAIR cross-entropy builds on MI355X: cutmix and unmixed batches
bit for bit the augmenting gather's pixels of the chosen source (both builds, crop + flip
plans), mixup per element within the derived bound of the float64 oracle (tests/mix_cases.py;
no element is skipped), the PAIR loss and dlogits within their bounds, the binding checks, the
GPU loader against the CPU loader, and a graphed ResNet-18 run whose replays follow each
step's own weights.

Shapes as tests/test_augment_gpu.py: 12 x 20 and 7 x 5, batches of 1 and 5 with a repeated
index, the first and the last image of the allocation as own and as partner (their windows
leave the allocation: the byte-load fallback), outputs NaN-filled between sentinel bands, on
and off the 16-byte grid."""
import pytest
import torch

import augment_cases as AC
import label_smoothing_cases as LS
import mix_cases as MC
from ddp_amd.data import (IMAGENET_MEAN, IMAGENET_STD, Augment, DeviceImageLoader, DeviceImages, Mix, PairTarget,
                          apply_reference)
from ddp_amd.data.mix import MIXUP
from elementwise import BF, F32, Guarded, bits

pytestmark = pytest.mark.gpu
dev = "cuda"
SHAPES = [(12, 20), (7, 5)]
N = 9
BATCHES = [[N - 1], [0, 1, 2, 3, 0], [4, 5, 6, 7, 4], [N - 1, 0, N - 1, 3, N - 1]]


def plan_rows(resample, H, W, seed=4):
    aug = Augment(rrc=True, flip=True, seed=seed) if resample else Augment(crop_pad=3, flip=True, seed=seed)
    rows = aug.plan(0, N, H, W).rows
    rows[0, 4], rows[N - 1, 4] = 1, 0  # the first image flipped, the last one not
    return rows


def guarded_out(B, H, W, skew):
    return Guarded((B, H, W, 4), BF, guard=4096, skew=skew)


def finish(out):
    torch.cuda.synchronize()
    out.check("the output")
    assert bool(torch.isfinite(out.t.float()).all()), "unwritten elements"
    assert bool((out.t[..., 3] == 0).all()), "4th channel"
    return out.t[..., :3].float().cpu()


def aug_gather(C, imgs, rows, aff, resample, idx, skew):
    out = guarded_out(len(idx), imgs.shape[1], imgs.shape[2], skew)
    C.image_gather_aug_nhwc4(imgs.to(dev), torch.as_tensor(idx).to(dev), rows.to(dev), aff, out.t, resample)
    return finish(out)


def mix_gather(C, imgs, rows, aff, resample, idx, tab, skew):
    out = guarded_out(len(idx), imgs.shape[1], imgs.shape[2], skew)
    C.image_gather_mix_nhwc4(imgs.to(dev), torch.as_tensor(idx).to(dev), rows.to(dev), aff, tab.to(dev), out.t,
                             resample)
    return finish(out)


# ------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("resample", [False, True])
def test_cutmix_and_unmixed_batches_copy_the_augmenting_gathers_pixels(C, H, W, resample):
    imgs, rows = AC.images(N, H, W, seed=3), plan_rows(resample, H, W)
    for aff in (AC.IMAGENET_AFFINE, AC.NEG_AFFINE):
        for skew, idx in enumerate(BATCHES):
            B = len(idx)
            own = aug_gather(C, imgs, rows, aff, resample, idx, skew % 2)
            for name, box in MC.box_cases(H, W):
                tab = MC.table(B, box, 1.0)
                got = mix_gather(C, imgs, rows, aff, resample, idx, tab, skew % 2)
                want = torch.where(MC.in_box(tab, H, W)[..., None], own.roll(1, 0), own)
                assert torch.equal(got, want), (name, idx, resample)
            # a weight of exactly 0 shows the partner everywhere, bit for bit
            got = mix_gather(C, imgs, rows, aff, resample, idx, MC.table(B, (0, 0, 0, 0), 0.0), skew % 2)
            assert torch.equal(got, own.roll(1, 0)), ("wa = 0", idx, resample)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("resample", [False, True])
def test_mixup_is_within_the_derived_bound(C, H, W, resample):
    imgs, rows = AC.images(N, H, W, seed=4), plan_rows(resample, H, W, seed=5)
    worst = 0.0
    for aff in (AC.IMAGENET_AFFINE, AC.NEG_AFFINE):
        ref = apply_reference(imgs, rows, aff, resample)
        err = MC.norm_error(imgs, rows, aff, resample, ref)
        for lam in (0.3, 0.98765, 2.0 ** -30):
            wa = torch.tensor(lam, dtype=torch.float64).float().item()
            for skew, idx in enumerate(BATCHES):
                B = len(idx)
                mref, bound = MC.mixup_bound(ref[idx], ref[idx].roll(1, 0), err[idx], err[idx].roll(1, 0), lam)
                got = mix_gather(C, imgs, rows, aff, resample, idx, MC.table(B, (0, 0, 0, 0), wa), skew % 2)
                worst = max(worst, MC.worst_ratio(got, mref, bound))
                # blending outside a box, the partner inside it
                box = (1, 1, W - 1, H - 2)
                tab = MC.table(B, box, wa)
                inb = MC.in_box(tab, H, W)[..., None]
                got = mix_gather(C, imgs, rows, aff, resample, idx, tab, skew % 2)
                own = aug_gather(C, imgs, rows, aff, resample, idx, skew % 2)
                assert torch.equal(got[inb.expand_as(got)], own.roll(1, 0)[inb.expand_as(got)])
                r = ((got.double() - mref).abs() / (bound + 1e-300))[(~inb).expand_as(got)]
                worst = max(worst, float(r.max()) if r.numel() else 0.0)
    print(f"{H}x{W} resample={resample}: mixup kernel error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_gather_binding_checks_the_table_and_skips_an_empty_batch(C):
    H, W = 7, 5
    imgs = AC.images(N, H, W).to(dev)
    rows = plan_rows(False, H, W).to(dev)
    out = torch.empty(2, H, W, 4, dtype=BF, device=dev)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    tab = MC.table(2, (0, 0, 2, 2), 1.0).to(dev)
    wide = torch.zeros(2, 12, dtype=torch.int32, device=dev)
    for bad in (tab[:, :5].contiguous(), tab[:1], tab.long(), tab.cpu(), tab.float(), wide[:, ::2]):
        with pytest.raises(RuntimeError):
            C.image_gather_mix_nhwc4(imgs, idx, rows, AC.PLAIN_AFFINE, bad, out, False)
    with pytest.raises(RuntimeError):
        C.image_gather_mix_nhwc4(imgs, idx, rows[:, :4].contiguous(), AC.PLAIN_AFFINE, tab, out, False)
    with pytest.raises(RuntimeError):
        C.image_gather_mix_nhwc4(imgs, idx, rows, AC.PLAIN_AFFINE.to(dev), tab, out, False)
    C.image_gather_mix_nhwc4(imgs, idx[:0], rows, AC.PLAIN_AFFINE, tab[:0], out[:0], False)  # no launch
    with pytest.raises(ValueError, match="partner"):  # refused on the host, before any upload
        MC.table(2, (0, 0, 0, 0), 1.0, partner=torch.tensor([0, 2]))


# -------------------------------------------------------------------------------------- loss
def run_xent(C, lg, ya, eps, what, yb=None, w=None, G=1, part=None, bias=None, extras=False, dbias_scale=0.0):
    B, NC = lg.shape
    dl, loss = Guarded((B, NC), F32), Guarded((1,), F32)
    lo = Guarded((B, NC), F32) if extras else None
    db = Guarded((NC,), F32) if extras else None
    kw = {"label_smoothing": eps} if eps else {}
    if yb is not None:
        kw.update(labels_b=yb, pair_w=w)
    C.xent(lg if part is None else part, G, bias, ya, lo.t if lo else None, dl.t, loss.t, db.t if db else None,
           LS.f32(1.0 / B), dbias_scale, **kw)
    torch.cuda.synchronize()
    for o in (dl, loss, lo, db):
        if o is not None:
            o.check(what)
    return dl.t, loss.t, lo.t if lo else None, db.t if db else None


def held(name, out, ref, bound, what):
    ok, r = LS.within(out, ref, bound)
    print(f"MIX_RATIO {what} {name} {r:.4f}")
    assert ok, f"{what}: {name} error / bound = {r:.3f} (or unwritten / non-finite elements)"


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("NC", [10, 65, 1000])
@pytest.mark.parametrize("E", [0.0, 0.1])
def test_pair_loss_is_within_the_bounds(C, B, NC, E):
    """NC = 10: xent_kernel; 65 / 1000: xent_wave_rows_kernel (B = 5: a partial block of 4 rows).
    Rows offset by 1e4, rows with y_a == y_b, wa in {0, 1, 0.3}."""
    for wa in (0.0, 1.0, 0.3):
        lg, ya, yb, w = (t.to(dev) for t in MC.pair_inputs(B, NC, wa))
        what = f"pair xent {(B, NC)} E={E} wa={wa}"
        dl, loss, _, _ = run_xent(C, lg, ya, E, what, yb, w)
        loss_ref, dl_ref, bl, bd = MC.pair_bounds(lg, ya, yb, w, LS.f32(E), LS.f32(1.0 / B))
        held("dlogits", dl, dl_ref, bd, what)
        held("loss", loss, loss_ref, bl, what)
        dl2, loss2, _, _ = run_xent(C, lg, ya, E, what, yb, w)
        assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(dl), bits(dl2)), f"{what}: two runs differ"
        if wa == 1.0:  # the build without pair targets, bit for bit
            dl0, loss0, _, _ = run_xent(C, lg, ya, E, what)
            assert torch.equal(bits(dl), bits(dl0)) and torch.equal(bits(loss), bits(loss0)), what


@pytest.mark.parametrize("E", [0.0, 0.1])
def test_pair_block_kernel_with_partials_bias_logits_and_dbias(C, E):
    B, G, NC, scale = 5, 3, 10, 0.25
    gen = torch.Generator().manual_seed(71)
    part = (torch.randn(B, G, NC, generator=gen) * 0.7).to(dev)
    bias = (torch.randn(NC, generator=gen) * 0.2).to(dev)
    ya = torch.tensor([NC - 1, 0, 3, 7, 3], device=dev)
    yb = torch.tensor([3, 0, NC - 1, 2, 3], device=dev)
    w = torch.tensor([[0.3, 0.7]], dtype=F32).expand(B, 2).contiguous().to(dev)
    what = f"pair xent block G=3 E={E}"
    shape = torch.empty(B, NC)
    dl, loss, lo, db = run_xent(C, shape, ya, E, what, yb, w, G=G, part=part, bias=bias, extras=True, dbias_scale=scale)
    x = part.cpu()
    lref = ((x[:, 0] + x[:, 1]) + x[:, 2]) + bias.cpu()
    assert torch.equal(bits(lo), bits(lref)), f"{what}: logits_out"
    loss_ref, dl_ref, bl, bd = MC.pair_bounds(lo, ya, yb, w, LS.f32(E), LS.f32(1.0 / B))
    held("dlogits", dl, dl_ref, bd, what)
    held("loss", loss, loss_ref, bl, what)
    d = dl.cpu()
    want = ((((d[0] + d[4]) + d[1]) + d[2]) + d[3]) * torch.tensor(scale, dtype=F32)
    assert torch.equal(bits(db), bits(want)), f"{what}: dbias is not the in-order sum of the stored dlogits"


@pytest.mark.parametrize("NC", [65, 1000])
@pytest.mark.parametrize("E", [0.0, 0.1])
@pytest.mark.parametrize("pair", [False, True])
def test_wave_and_block_kernels_agree(C, NC, E, pair):
    """The same [5, NC] logits through xent_wave_rows_kernel (the plain call) and through
    xent_kernel (the same call with logits_out and dbias, which routes there), in all four builds:
    both evaluate the one row body of csrc/kernels/xent_body.h, so dlogits agree bit for bit.  The
    mean losses are summed in different orders (rows in order; per wave, then over the waves), so
    each is held to the loss bound of its build instead."""
    B = 5
    lg, ya, yb, w = (t.to(dev) for t in MC.pair_inputs(B, NC, 0.3))
    tgt = (yb, w) if pair else (None, None)
    what = f"wave / block xent {(B, NC)} E={E} pair={pair}"
    dlw, lw, _, _ = run_xent(C, lg, ya, E, what + " wave", *tgt)
    dlb, lb, _, _ = run_xent(C, lg, ya, E, what + " block", *tgt, extras=True)
    assert torch.equal(bits(dlw), bits(dlb)), f"{what}: the two kernels' dlogits differ"
    if pair:
        loss_ref, _, bl, _ = MC.pair_bounds(lg, ya, yb, w, LS.f32(E), LS.f32(1.0 / B))
    else:
        loss_ref, _, bl, _ = LS.bounds(lg, ya, LS.f32(E), LS.f32(1.0 / B))
    held("wave loss", lw, loss_ref, bl, what)
    held("block loss", lb, loss_ref, bl, what)


def test_xent_binding_checks_the_pair_arguments(C):
    B, NC = 3, 65
    lg, ya, yb, w = (t.to(dev) for t in MC.pair_inputs(B, NC, 0.3))
    dl, loss = torch.empty(B, NC, device=dev), torch.empty(1, device=dev)

    def call(labels, **kw):
        C.xent(lg, 1, None, labels, None, dl, loss, None, 1.0 / B, 0.0, **kw)

    call(ya, labels_b=yb, pair_w=w)
    for bad in (dict(labels_b=yb), dict(pair_w=w), dict(labels_b=yb.int(), pair_w=w), dict(labels_b=yb, pair_w=w.double()),
                dict(labels_b=yb[:2], pair_w=w), dict(labels_b=yb, pair_w=w[:, :1].contiguous()),
                dict(labels_b=yb.cpu(), pair_w=w), dict(labels_b=yb, pair_w=w.t().contiguous().t())):
        with pytest.raises((RuntimeError, ValueError)):
            call(ya, **bad)
    with pytest.raises((RuntimeError, ValueError)):  # the fused engine's int32 label source has no pair build
        call(ya.int(), labels_b=yb, pair_w=w)


def test_module_loss_takes_a_pair_target_and_backpropagates(C):
    from ddp_amd.ops import CrossEntropyLoss

    B, NC = 5, 1000
    lg, ya, yb, w = (t.to(dev) for t in MC.pair_inputs(B, NC, 0.3))
    lg.requires_grad_(True)
    loss = CrossEntropyLoss(0.1)(lg, PairTarget(ya, yb, w))
    loss.backward()
    loss_ref, dl_ref, bl, bd = MC.pair_bounds(lg, ya, yb, w, LS.f32(0.1), LS.f32(1.0 / B))
    held("dlogits", lg.grad, dl_ref, bd, "module loss")
    held("loss", loss.reshape(1), loss_ref, bl, "module loss")


# ------------------------------------------------------------------------------------ loader
@pytest.mark.parametrize("mode", ["crop", "rrc"])
def test_loader_yields_the_cpu_loaders_batches(mode):
    """Two epochs, ragged last batch (37 images, batch 8), normalised: cutmix and unmixed batches
    of the integer build bit for bit, everything else within the bound of the float64 oracle."""
    n, H, W = 37, 12, 20
    imgs, labels = AC.images(n, H, W, seed=5), torch.arange(n) % 10
    resample = mode == "rrc"
    aug = Augment(rrc=True, flip=True, seed=2) if resample else Augment(crop_pad=3, flip=True, seed=2)
    mix = Mix(0.2, 1.0, seed=3)
    norm = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD)
    g = DeviceImageLoader(DeviceImages(imgs, labels, dev, **norm), 8, 1, 0, augment=aug, mix=mix)
    c = DeviceImageLoader(DeviceImages(imgs, labels, "cpu", **norm), 8, 1, 0, augment=aug, mix=mix)
    modes = set()
    for epoch in (0, 1):
        g.sampler.set_epoch(epoch)
        c.sampler.set_epoch(epoch)
        rows = aug.plan(epoch, n, H, W).rows
        mp = mix.plan(epoch, 0, len(c), H, W)
        idx = c.sampler.indices()
        sizes = []
        for step, ((xg, tg), (xc, tc)) in enumerate(zip(g, c)):
            assert isinstance(tg, PairTarget) and all(torch.equal(a.cpu(), b) for a, b in zip(tg, tc))
            assert xg.dtype == BF and bool((xg[..., 3] == 0).all())
            got, host = xg[..., :3].float().cpu(), xc.permute(0, 2, 3, 1)
            sizes.append(len(tc.y_a))
            modes.add(int(mp.mode[step]))
            bidx = idx[step * 8:step * 8 + 8]
            ref = apply_reference(imgs[bidx], rows[bidx], AC.IMAGENET_AFFINE, resample)
            err = MC.norm_error(imgs[bidx], rows[bidx], AC.IMAGENET_AFFINE, resample, ref)
            if int(mp.mode[step]) == MIXUP:
                mref, bound = MC.mixup_bound(ref, ref.roll(1, 0), err, err.roll(1, 0), float(mp.lam[step]))
            else:
                inb = MC.in_box(mp.rows_for(step, len(bidx))[0], H, W)[..., None]
                mref = torch.where(inb, ref.roll(1, 0), ref)
                e = torch.where(inb, err.roll(1, 0), err)
                bound = e * (1 + 2.0 ** -8) + 2.0 ** -8 * mref.abs()
                if not resample:
                    assert torch.equal(got, host), (epoch, step)
            assert MC.worst_ratio(got, mref, bound) <= 1.0 and MC.worst_ratio(host, mref, bound) <= 1.0
        assert sizes == [8, 8, 8, 8, 5]
    assert len(modes) >= 2


# ------------------------------------------------------------------------------ graphed step
def _losses(graph, seed, epochs=2):
    from ddp_amd.data import synthetic_imagenet
    from ddp_amd.engine.trainer import _run_module_epoch
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    torch.manual_seed(0)
    model = resnet18(num_classes=10).to(dev)
    model.train()
    opt = FusedSGD(model, lr=0.01, momentum=0.9)
    imgs, labels = synthetic_imagenet(16, 64, 10)
    data = DeviceImages(imgs, labels, dev, mean=IMAGENET_MEAN, std=IMAGENET_STD)
    mix = Mix(0.2, 1.0, seed=seed)
    loader = DeviceImageLoader(data, 4, 1, 0, augment=Augment(rrc=True, flip=True), mix=mix)
    out, weights = [], []
    for epoch in range(epochs):
        loader.sampler.set_epoch(epoch)
        weights += mix.plan(epoch, 0, len(loader), 64, 64).wa.tolist()
        _run_module_epoch(model, loader, CrossEntropyLoss(0.1), opt, torch.device(dev), lambda i, v: out.append(v), 1,
                          None, graph=graph)
    torch.cuda.synchronize()
    return out, weights


def test_graphed_step_replays_each_steps_own_weights():
    """ResNet-18 at 64 x 64, batch 4, both alphas, --graph_module: step 0 captures, the other seven
    replay with their own weights (read from the static inputs on the device): the per-step
    losses differ and are the eager run's bit for bit; another seed gives other losses."""
    eager, weights = _losses(False, 1)
    graphed, _ = _losses(True, 1)
    assert len(eager) == 8 and len(set(weights)) > 2
    assert eager == graphed
    assert len(set(graphed)) == 8
    other, _ = _losses(True, 2)
    assert other != graphed
