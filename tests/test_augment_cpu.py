"""On-device train augmentation, the host side: the per-epoch plan (a pure function of seed,
epoch and data-set index), the float64 oracle pinned to torch's own pad / slice / flip /
interpolate, the a-priori rounding bound of the bilinear build (tests/augment_cases.py) met by
the fp32 host path and missed by five wrong implementations, and the CPU trainer (resume is
bitwise, the flags change the run, the refusals raise)."""
import os

import pytest
import torch
import torch.multiprocessing as mp

import augment_cases as AC
from ddp_amd.data import (AugPlan, Augment, DeviceImageLoader, DeviceImages, apply_fp32, apply_reference,
                          epoch_indices)
from ddp_amd.parallel import free_port


# ------------------------------------------------------------------ plan properties
def test_plan_is_deterministic_and_differs_between_epochs():
    a = Augment(rrc=True, flip=True, seed=3)
    p0, p0b, p1 = a.plan(0, 37, 12, 20), Augment(rrc=True, flip=True, seed=3).plan(0, 37, 12, 20), a.plan(1, 37, 12, 20)
    assert p0.rows.dtype == torch.int32 and tuple(p0.rows.shape) == (37, 5) and p0.resample
    assert torch.equal(p0.rows, p0b.rows)
    assert not torch.equal(p0.rows, p1.rows)
    assert not torch.equal(p0.rows, Augment(rrc=True, flip=True, seed=4).plan(0, 37, 12, 20).rows)


def test_plan_rows_do_not_depend_on_world_or_batch_size():
    """An image's row is looked up by its data-set index: whichever rank and batch the sampler
    puts it in, and however often the wrap-around repeats it, it is the same row."""
    n, H, W = 37, 12, 20
    imgs = AC.images(n, H, W)
    labels = torch.arange(n)  # the label IS the data-set index
    aug = Augment(crop_pad=2, flip=True, seed=1)
    plan = aug.plan(5, n, H, W)
    want = apply_fp32(imgs, plan.rows, AC.PLAIN_AFFINE).permute(0, 3, 1, 2)
    data = DeviceImages(imgs, labels, "cpu")
    for ws, bs in ((1, 8), (2, 5), (3, 4)):
        seen = 0
        for rank in range(ws):
            ld = DeviceImageLoader(data, bs, ws, rank, augment=aug)
            ld.sampler.set_epoch(5)
            got_idx = []
            for x, y in ld:
                assert torch.equal(x, want[y]), (ws, bs, rank)
                got_idx.append(y)
            assert torch.equal(torch.cat(got_idx), epoch_indices(n, ws, rank, 5))
            seen += sum(t.numel() for t in got_idx)
        assert seen >= n  # (wrap-around duplicates included: they matched the same rows)


def test_plan_stream_is_not_the_samplers():
    a = Augment(crop_pad=2, seed=0)
    for seed, epoch in ((0, 0), (0, 1), (1, 0), (7, 3)):
        a.seed = seed
        assert a.stream_seed(epoch) != seed + epoch
    a.seed = 0
    assert Augment(seed=1).stream_seed(0) != a.stream_seed(1)  # equal sums, different streams
    n = 64
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0 + 2))
    mine = torch.randperm(n, generator=torch.Generator().manual_seed(a.stream_seed(2)))
    assert not torch.equal(perm, mine)


# ------------------------------------------------------------------ ranges
def test_crop_offsets_cover_their_range():
    P = 2
    rows = Augment(crop_pad=P, seed=0).plan(0, 4096, 8, 8).rows
    for col in (0, 1):
        d = rows[:, col] + P
        assert int(d.min()) == 0 and int(d.max()) == 2 * P
    assert bool((rows[:, 2] == 8).all()) and bool((rows[:, 3] == 8).all()) and bool((rows[:, 4] == 0).all())


def test_rrc_boxes_lie_inside_the_image():
    for H, W, smin in ((12, 20, 0.08), (7, 5, 0.08), (224, 224, 0.08), (12, 20, 1.0)):
        r = Augment(rrc=True, scale=(smin, 1.0), seed=2).plan(0, 4096, H, W).rows.long()
        top, left, h, w = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
        assert bool(((h >= 1) & (h <= H) & (w >= 1) & (w <= W)).all())
        assert bool(((top >= 0) & (top + h <= H) & (left >= 0) & (left + w <= W)).all())


def test_flip_frequency():
    n = 4096
    f = Augment(flip=True, seed=0).plan(0, n, 8, 8).rows[:, 4].double()
    assert set(f.tolist()) == {0.0, 1.0}
    assert abs(float(f.mean()) - 0.5) <= 5 * 0.5 / n ** 0.5


def test_rrc_fallback_is_the_central_crop():
    """4 x 40 with scale >= 0.9: every try wants h of about 10 or more rows, none fits, and the
    fallback clamps the ratio: h = 4, w = round(4 * 4/3) = 5, centred."""
    rows = Augment(rrc=True, scale=(0.9, 1.0), seed=0).plan(0, 50, 4, 40).rows
    assert torch.equal(rows[:, :4], torch.tensor([[0, 17, 4, 5]], dtype=torch.int32).expand(50, 4))
    tall = Augment(rrc=True, scale=(0.9, 1.0), seed=0).plan(0, 5, 40, 4).rows
    assert torch.equal(tall[:, :4], torch.tensor([[17, 0, 5, 4]], dtype=torch.int32).expand(5, 4))


def test_augment_refuses_bad_recipes():
    with pytest.raises(ValueError):
        Augment(crop_pad=2, rrc=True)
    with pytest.raises(ValueError):
        Augment(rrc=True, scale=(0.0, 1.0))
    with pytest.raises(ValueError):
        Augment(crop_pad=5).plan(0, 4, 7, 5)


# ------------------------------------------------------------------ the oracle against torch
@pytest.mark.parametrize("H,W", [(12, 20), (7, 5)])
def test_reference_integer_build_is_torch_pad_slice_flip(H, W):
    rows = AC.shift_rows(H, W, P=3)
    imgs = AC.images(len(rows), H, W)
    for aff in (AC.IMAGENET_AFFINE, AC.NEG_AFFINE, AC.PLAIN_AFFINE):
        assert torch.equal(apply_reference(imgs, rows, aff), AC.torch_reference_batch(imgs, rows, aff, False))


@pytest.mark.parametrize("H,W", [(12, 20), (7, 5)])
def test_reference_bilinear_build_is_torch_interpolate(H, W):
    rows = torch.cat([AC.box_rows(H, W), Augment(rrc=True, flip=True, seed=1).plan(0, 9, H, W).rows])
    imgs = AC.images(len(rows), H, W, seed=1)
    got = apply_reference(imgs, rows, AC.IMAGENET_AFFINE, True)
    want = AC.torch_reference_batch(imgs, rows, AC.IMAGENET_AFFINE, True)
    assert float((got - want).abs().max()) <= 1e-12
    one = rows[:, 2] * rows[:, 3] == 1  # a 1 x 1 box: the whole output is that pixel
    px = imgs[one, rows[one, 0].long(), rows[one, 1].long()].double() * AC.IMAGENET_AFFINE[:, 0].double() \
        + AC.IMAGENET_AFFINE[:, 1].double()
    assert torch.equal(got[one], px[:, None, None, :].expand(-1, H, W, -1))


def test_identity_plan_reproduces_the_plain_gather():
    imgs = AC.images(9, 12, 20)
    want = (imgs.float() * (1.0 / 255.0)).to(torch.bfloat16).float()  # the plain kernel's v * (1.f / 255.f)
    for resample in (False, True):
        rows = AugPlan.identity(9, 12, 20, resample).rows
        assert torch.equal(apply_fp32(imgs, rows, AC.PLAIN_AFFINE, resample), want)


# ------------------------------------------------------------------ the bound
def _bilinear_case(H, W, seed=2):
    rows = torch.cat([AC.box_rows(H, W), Augment(rrc=True, flip=True, seed=seed).plan(0, 9, H, W).rows])
    imgs = AC.images(len(rows), H, W, seed=seed)
    return imgs, rows


@pytest.mark.parametrize("H,W", [(12, 20), (7, 5), (12, 12)])
def test_fp32_bilinear_path_meets_the_derived_bound(H, W):
    imgs, rows = _bilinear_case(H, W)
    for aff in (AC.IMAGENET_AFFINE, AC.NEG_AFFINE):
        ref = apply_reference(imgs, rows, aff, True)
        r = AC.worst_ratio(apply_fp32(imgs, rows, aff, True), ref, AC.bilinear_bound(imgs, rows, aff, ref))
        print(f"{H}x{W}: fp32 host path error / bound = {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("variant", ["align_corners", "swap_weights", "flip_first", "nearest"])
def test_wrong_bilinear_implementations_miss_the_bound(variant):
    imgs, rows = _bilinear_case(12, 12)
    aff = AC.IMAGENET_AFFINE
    ref = apply_reference(imgs, rows, aff, True)
    bound = AC.bilinear_bound(imgs, rows, aff, ref)
    wrong = AC.to_bf16(AC.torch_reference_batch(imgs, rows, aff, True, variant))
    assert AC.worst_ratio(wrong, ref, bound) > 1.0
    right = AC.to_bf16(AC.torch_reference_batch(imgs, rows, aff, True))
    assert AC.worst_ratio(right, ref, bound) <= 1.0  # (the same route with the right formula passes)


def test_padding_after_the_normalisation_is_caught():
    """The padding is a black pixel BEFORE the fma (b_c, not 0, after it): integer build, exact."""
    rows = AC.shift_rows(12, 20)
    imgs = AC.images(len(rows), 12, 20)
    aff = AC.IMAGENET_AFFINE
    got = apply_fp32(imgs, rows, aff)
    assert torch.equal(got.double(), AC.to_bf16(AC.torch_reference_batch(imgs, rows, aff, False)))
    assert not torch.equal(got.double(), AC.to_bf16(AC.torch_reference_batch(imgs, rows, aff, False, "pad_after_norm")))
    pad = apply_fp32(torch.zeros(1, 12, 20, 3, dtype=torch.uint8), rows[:1], aff)  # a black image: all b_c
    assert torch.equal(pad[0, 0, 0], aff[:, 1].to(torch.bfloat16).float())


# ------------------------------------------------------------------ the CPU trainer
def _opts(ckdir, **kw):
    from ddp_amd.engine.trainer import TrainOptions

    return TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, log_every=100, model="resnet18",
                        image_size=32, num_classes=10, dataset_size=24, momentum=0.9, **kw)


def _worker(rank, port, ckdir, epochs, kw, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import ddp_train

    model = ddp_train(rank, 1, epochs, 8, _opts(ckdir, **kw))
    q.put({n: p.detach().cpu().numpy().copy() for n, p in model.state_dict().items()})  # (plain arrays: the
    # producer exits before the reader maps a shared tensor)


def _train(ckdir, epochs, **kw):
    q = mp.get_context("spawn").Queue()
    p = mp.get_context("spawn").Process(target=_worker, args=(0, free_port(), str(ckdir), epochs, kw, q))
    p.start()
    out = q.get(timeout=600)
    p.join(timeout=60)
    return out


@pytest.mark.slow
def test_cpu_trainer_resume_is_bitwise_and_the_flags_change_the_run(tmp_path):
    aug = dict(aug_rrc=True, aug_flip=True, normalize=True)
    two = _train(tmp_path / "a", 2, **aug)
    _train(tmp_path / "b", 1, **aug)
    resumed = _train(tmp_path / "b", 2, **aug)  # epoch 1 alone, from epoch 0's checkpoint
    assert sorted(os.listdir(tmp_path / "b")) == ["epoch_0.pt", "epoch_1.pt"]
    for n in two:
        assert two[n].tobytes() == resumed[n].tobytes(), n
    plain = _train(tmp_path / "c", 2)
    assert any(two[n].tobytes() != plain[n].tobytes() for n in two)


def test_option_refusals():
    from ddp_amd.engine.trainer import TrainOptions, augment_tag, validate_options

    validate_options(_opts("x", aug_rrc=True, aug_flip=True, normalize=True))
    validate_options(_opts("x", aug_crop_pad=4))
    for bad in (dict(aug_crop_pad=4, aug_rrc=True), dict(aug_crop_pad=32), dict(aug_crop_pad=-1),
                dict(aug_rrc=True, aug_scale_min=0.0), dict(aug_rrc=True, aug_scale_min=1.5)):
        with pytest.raises(ValueError):
            validate_options(_opts("x", **bad))
    for flag in (dict(normalize=True), dict(aug_flip=True), dict(aug_rrc=True), dict(aug_crop_pad=2)):
        with pytest.raises(ValueError, match="resnet18"):
            validate_options(TrainOptions(model="simplecnn", **flag))
    assert augment_tag(_opts("x", aug_rrc=True, aug_flip=True, normalize=True)) == "rrc+flip+norm"
    assert augment_tag(_opts("x", aug_crop_pad=4)) == "crop4" and augment_tag(_opts("x")) == ""


def test_cli_flags_reach_the_options():
    import train_ddp

    a = train_ddp.parse_args(["--model", "resnet18", "--aug_crop_pad", "4", "--aug_flip", "--normalize"])
    assert a.aug_crop_pad == 4 and a.aug_flip and a.normalize and not a.aug_rrc and a.aug_scale_min == 0.08
