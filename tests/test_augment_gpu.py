"""image_gather_aug_nhwc4 on MI355X: both builds against the plain gather (identity plan), the
integer build bit for bit against the host path, the bilinear build per element against the
float64 oracle within the derived bound (tests/augment_cases.py; no element is skipped), the
loader against the CPU loader, and graphed training with the flags on.

Shapes: 12 x 20 (non-square: a row/column swap shows) and 7 x 5 (narrower than two 4-pixel
runs, odd: the 3-byte pixels' dword alignment and the rows' 16-byte alignment change from row
to row).  Every output is NaN-filled inside a larger allocation whose sentinel bands must
stay untouched."""
import json

import pytest
import torch

import augment_cases as AC
from ddp_amd.data import (IMAGENET_MEAN, IMAGENET_STD, AugPlan, Augment, DeviceImageLoader, DeviceImages, apply_fp32,
                          apply_reference)
from elementwise import BF, Guarded

pytestmark = pytest.mark.gpu
dev = "cuda"
SHAPES = [(12, 20), (7, 5)]
N = 9


def gather(C, imgs, rows, affine, resample, idx, skew=0):
    """The kernel on images ``imgs`` with the table ``rows`` (one per data-set image), into a
    NaN-filled output between two bands of 4096 sentinels; ``skew`` moves it by 4 elements, so its
    base is 8- but not 16-byte aligned."""
    out = Guarded((len(idx), imgs.shape[1], imgs.shape[2], 4), BF, guard=4096, skew=skew)
    C.image_gather_aug_nhwc4(imgs.to(dev), torch.as_tensor(idx).to(dev), rows.to(dev), affine, out.t, resample)
    torch.cuda.synchronize()
    out.check("the output")
    assert bool(torch.isfinite(out.t.float()).all()), "unwritten elements"
    assert bool((out.t[..., 3] == 0).all()), "4th channel"
    return out.t[..., :3].float().cpu()


def batches(n):
    """A batch of 1 and batches of 5 with a repeated index, covering every image."""
    order = list(range(n))
    out = [[n - 1]]
    for s in range(0, n, 4):
        out.append((order[s:s + 4] + [order[s]] * 5)[:5])
    return out


@pytest.mark.parametrize("H,W", SHAPES)
def test_identity_plan_equals_the_plain_gather(C, H, W):
    imgs = AC.images(N, H, W)
    for resample in (False, True):
        rows = AugPlan.identity(N, H, W).rows
        for skew, idx in enumerate(batches(N)):
            plain = torch.full((len(idx), H, W, 4), float("nan"), dtype=BF, device=dev)
            C.image_gather_nhwc4(imgs.to(dev), torch.tensor(idx, device=dev), plain)
            got = gather(C, imgs, rows, AC.PLAIN_AFFINE, resample, idx, skew % 2)
            assert torch.equal(got, plain[..., :3].float().cpu()), (resample, idx)


@pytest.mark.parametrize("H,W", SHAPES)
def test_integer_build_is_bitwise_the_host_path(C, H, W):
    rows = AC.shift_rows(H, W, P=3)  # 9 offsets x {no flip, flip}: one row per image
    imgs = AC.images(len(rows), H, W, seed=3)
    for aff in (AC.IMAGENET_AFFINE, AC.NEG_AFFINE):
        want = apply_fp32(imgs, rows, aff)
        for skew, idx in enumerate(batches(len(rows))):
            got = gather(C, imgs, rows, aff, False, idx, skew % 2)
            assert torch.equal(got, want[idx]), (idx, aff)


@pytest.mark.parametrize("H,W", SHAPES)
def test_bilinear_build_is_within_the_derived_bound(C, H, W):
    rows = torch.cat([AC.box_rows(H, W), Augment(rrc=True, flip=True, seed=4).plan(0, N, H, W).rows])
    imgs = AC.images(len(rows), H, W, seed=4)
    for aff in (AC.IMAGENET_AFFINE, AC.NEG_AFFINE):
        ref = apply_reference(imgs, rows, aff, True)
        bound = AC.bilinear_bound(imgs, rows, aff, ref)
        worst = 0.0
        for skew, idx in enumerate(batches(len(rows))):
            got = gather(C, imgs, rows, aff, True, idx, skew % 2)
            worst = max(worst, AC.worst_ratio(got, ref[idx], bound[idx]))
        print(f"{H}x{W}: bilinear kernel error / bound = {worst:.3f}")
        assert worst <= 1.0


def test_binding_checks_the_table_and_skips_an_empty_batch(C):
    imgs = AC.images(N, 7, 5).to(dev)
    rows = AugPlan.identity(N, 7, 5).rows.to(dev)
    out = torch.empty(1, 7, 5, 4, dtype=BF, device=dev)
    idx = torch.zeros(1, dtype=torch.int64, device=dev)
    for bad in (rows[:, :4].contiguous(), rows[:N - 1], rows.long(), rows.cpu()):
        with pytest.raises(RuntimeError):
            C.image_gather_aug_nhwc4(imgs, idx, bad, AC.PLAIN_AFFINE, out, False)
    with pytest.raises(RuntimeError):
        C.image_gather_aug_nhwc4(imgs, idx, rows, AC.PLAIN_AFFINE.to(dev), out, False)
    C.image_gather_aug_nhwc4(imgs, idx[:0], rows, AC.PLAIN_AFFINE, out[:0], False)  # no launch


@pytest.mark.parametrize("mode", ["crop", "rrc"])
def test_loader_yields_the_cpu_loaders_batches(mode):
    """Two epochs, ragged last batch (37 images, batch 8), normalised: the integer build bit
    for bit, the bilinear build within the bound of the float64 oracle."""
    n, H, W = 37, 12, 20
    imgs, labels = AC.images(n, H, W, seed=5), torch.arange(n)
    aug = Augment(crop_pad=3, flip=True, seed=2) if mode == "crop" else Augment(rrc=True, flip=True, seed=2)
    norm = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD)
    g = DeviceImageLoader(DeviceImages(imgs, labels, dev, **norm), 8, 1, 0, augment=aug)
    c = DeviceImageLoader(DeviceImages(imgs, labels, "cpu", **norm), 8, 1, 0, augment=aug)
    for epoch in (0, 1):
        g.sampler.set_epoch(epoch)
        c.sampler.set_epoch(epoch)
        rows = aug.plan(epoch, n, H, W).rows
        sizes = []
        for (xg, yg), (xc, yc) in zip(g, c):
            assert torch.equal(yg.cpu(), yc) and xg.dtype == BF and bool((xg[..., 3] == 0).all())
            got = xg[..., :3].float().cpu()
            sizes.append(len(yc))
            if mode == "crop":
                assert torch.equal(got, xc.permute(0, 2, 3, 1))
            else:
                ref = apply_reference(imgs[yc], rows[yc], AC.IMAGENET_AFFINE, True)
                bound = AC.bilinear_bound(imgs[yc], rows[yc], AC.IMAGENET_AFFINE, ref)
                assert AC.worst_ratio(got, ref, bound) <= 1.0
                assert AC.worst_ratio(xc.permute(0, 2, 3, 1), ref, bound) <= 1.0
        assert sizes == [8, 8, 8, 8, 5]


def _trainer_worker(rank, port, ckdir, graph, q):
    import os

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        from ddp_amd.data import synthetic_imagenet_test
        from ddp_amd.engine.evaluation import evaluate_resnet
        from ddp_amd.engine.trainer import TrainOptions, ddp_train

        mj = os.path.join(ckdir, "metrics.jsonl")
        os.makedirs(ckdir, exist_ok=True)
        opts = TrainOptions(checkpoint_dir=ckdir, log_every=1, model="resnet18", image_size=64, num_classes=10,
                            dataset_size=40, momentum=0.9, graph_module=graph, aug_crop_pad=4, aug_flip=True,
                            normalize=True, eval_every=1, eval_size=16, eval_batch_size=8, metrics_json=mj)
        model = ddp_train(rank, 1, 1, 8, opts)
        rec = json.loads(open(mj).read().splitlines()[-1])
        # the held-out result again, from batches gathered and normalised on the CPU
        timgs, tlabels = synthetic_imagenet_test(16, 64, 10, n_train=40)
        norm = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD)
        gres = evaluate_resnet(model, DeviceImages(timgs, tlabels, "cuda", **norm), batch_size=8, want_logits=True)
        xc, _ = DeviceImages(timgs, tlabels, "cpu", **norm).gather(torch.arange(16))
        x4 = torch.zeros(16, 64, 64, 4, dtype=torch.bfloat16)
        x4[..., :3] = xc.permute(0, 2, 3, 1).to(torch.bfloat16)
        with torch.no_grad():
            folded = model.fold_bn()
            lg = torch.cat([model.forward_infer(x4[s:s + 8].cuda(), folded) for s in (0, 8)]).float()
        loss = (torch.logsumexp(lg, dim=1) - lg.gather(1, tlabels.cuda().view(-1, 1))[:, 0]).double().mean().item()
        q.put(("ok", dict(params=float(sum(p.detach().double().sum() for p in model.parameters())), rec=rec,
                          same_logits=bool(torch.equal(lg, gres.logits.float())),
                          gres=(gres.mean_loss, gres.accuracy), cpu_loss=loss,
                          cpu_acc=float((lg.argmax(1).cpu() == tlabels).double().mean()))))
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((repr(e) + traceback.format_exc(), None))


def test_graphed_training_with_augmentation_equals_eager(tmp_path):
    """--graph_module == eager bit for bit with --aug_crop_pad 4 --aug_flip --normalize (the
    gather runs before the replay and its result is copied into the static input), and the
    run's held-out evaluation is the one CPU-gathered, normalised batches give the same model:
    identical logits, hence the same accuracy, and the same loss up to the summation."""
    import torch.multiprocessing as mp

    from ddp_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    res = {}
    for graph in (False, True):
        q = ctx.Queue()
        p = ctx.Process(target=_trainer_worker, args=(0, free_port(), str(tmp_path / f"ck{int(graph)}"), graph, q))
        p.start()
        res[graph] = q.get(timeout=240)
        p.join(timeout=60)
        assert res[graph][0] == "ok", res[graph]
    e, g = res[False][1], res[True][1]
    assert e["params"] == g["params"]
    assert e["rec"]["eval_loss"] == g["rec"]["eval_loss"] and e["rec"]["eval_accuracy"] == g["rec"]["eval_accuracy"]
    for r in (e, g):
        assert r["rec"]["augment"] == "crop4+flip+norm"
        assert r["same_logits"]
        assert (r["rec"]["eval_loss"], r["rec"]["eval_accuracy"]) == r["gres"]
        assert r["cpu_acc"] == r["rec"]["eval_accuracy"]
        # the tail kernel and torch sum the same logits' exponentials in fp32 in different orders:
        # some tens of roundings of 2**-24 relative to logits of magnitude <= 2**5
        assert abs(r["cpu_loss"] - r["rec"]["eval_loss"]) <= 64 * 2.0 ** -24 * 32
