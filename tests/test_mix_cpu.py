"""Mixup / CutMix, the host side: the float64 oracle pinned to a literal roll / one_hot / slicing
implementation, the box rule, the per-batch plan (a pure function of seed, epoch, rank and
batch index), the CPU loss against F.cross_entropy with probability targets, the a-priori
bounds (tests/mix_cases.py) met by the fp32 host path and the emulated PAIR kernels and missed
by planted errors, the refusals, and a 2-rank CPU crash-and-resume run."""
import os

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import augment_cases as AC
import label_smoothing_cases as LS
import mix_cases as MC
from ddp_amd.data import (IMAGENET_MEAN, IMAGENET_STD, AugPlan, Augment, DeviceImageLoader, DeviceImages, Mix,
                          PairTarget, apply_fp32, apply_reference, mix_fp32, mix_reference, mix_table)
from ddp_amd.data.augment import normalized_fp32
from ddp_amd.data.mix import CUTMIX, MIXUP, NONE, cutmix_box
from ddp_amd.ops import CrossEntropyLoss
from ddp_amd.parallel import free_port

H, W = 12, 20


# ------------------------------------------------------------------ the oracle and the box rule
def test_reference_is_roll_onehot_slicing():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, H, W, 3, generator=g, dtype=torch.float64)
    y = torch.tensor([3, 1, 4, 1, 5])
    lam, E, C = 0.3, 0.1, 7
    out, t = mix_reference(x, y, C, MIXUP, None, lam, E)
    want = torch.stack([lam * x[b] + (1 - lam) * x[b - 1] for b in range(5)])  # x[-1]: the roll's wrap
    assert torch.equal(out, want)
    oh = torch.eye(C, dtype=torch.float64)[y] * (1 - E) + E / C
    assert torch.allclose(t, torch.stack([lam * oh[b] + (1 - lam) * oh[b - 1] for b in range(5)]), rtol=0, atol=1e-15)
    box = (2, 3, 9, 8)
    out, t = mix_reference(x, y, C, CUTMIX, box, 0.75, 0.0)
    for b in range(5):
        for r in range(H):
            for c in range(W):
                src = b - 1 if (3 <= r < 8 and 2 <= c < 9) else b
                assert torch.equal(out[b, r, c], x[src, r, c])
    assert torch.equal(t[0], 0.75 * torch.eye(C, dtype=torch.float64)[3] + 0.25 * torch.eye(C, dtype=torch.float64)[5])
    out, t = mix_reference(x, y, C, NONE, None, 1.0)
    assert torch.equal(out, x) and torch.equal(t, torch.eye(C, dtype=torch.float64)[y])
    one, t1 = mix_reference(x[:1], y[:1], C, MIXUP, None, 0.3)  # a batch of 1 mixes with itself
    assert torch.allclose(one, x[:1], rtol=0, atol=1e-15) and torch.allclose(t1, torch.eye(C, dtype=torch.float64)[y[:1]])


def test_box_rule_by_hand_and_at_the_clamps():
    # lam0 = 0.75: r = 0.5 * sqrt(0.25) = 0.25 -> hw = int(0.25 * 20) = 5, hh = int(0.25 * 12) = 3
    assert cutmix_box(0.75, 10, 6, H, W) == ((5, 3, 15, 9), 1.0 - 60.0 / 240.0)
    # clamped at the left / top: x in [0, 7), y in [0, 4) -> 28 pixels, lam from the clipped area
    box, lam = cutmix_box(0.75, 2, 1, H, W)
    assert box == (0, 0, 7, 4) and lam == 1.0 - 28.0 / 240.0 and lam != 0.75
    # clamped at the right / bottom
    box, lam = cutmix_box(0.75, 19, 11, H, W)
    assert box == (14, 8, 20, 12) and lam == 1.0 - 24.0 / 240.0
    # lam0 = 1: an empty box, lam exactly 1; lam0 = 0: half sizes W/2, H/2, the full image from the centre
    assert cutmix_box(1.0, 7, 7, H, W) == ((7, 7, 7, 7), 1.0)
    assert cutmix_box(0.0, 10, 6, H, W) == ((0, 0, 20, 12), 0.0)
    assert cutmix_box(0.0, 0, 0, H, W) == ((0, 0, 10, 6), 0.75)


def test_lam_exactly_zero_and_one_work():
    """A tiny alpha draws 0 and 1 exactly; the tables, the host path and the loss take them."""
    p = Mix(mixup_alpha=1e-3, seed=1).plan(0, 0, 64, H, W)
    lams = set(p.lam.tolist())
    assert 1.0 in lams and min(lams) < 1e-30 and all(0.0 <= v <= 1.0 for v in lams)
    imgs = AC.images(5, H, W)
    n32 = normalized_fp32(imgs, AugPlan.identity(5, H, W).rows, AC.IMAGENET_AFFINE)
    own = n32.to(torch.bfloat16).float()
    assert torch.equal(mix_fp32(n32, MC.table(5, (0, 0, 0, 0), 1.0)), own)
    assert torch.equal(mix_fp32(n32, MC.table(5, (0, 0, 0, 0), 0.0)), own.roll(1, 0))
    lg = torch.randn(5, 10, generator=torch.Generator().manual_seed(2))
    ya, yb = torch.arange(5), torch.arange(5).roll(1)
    for wa, y in ((1.0, ya), (0.0, yb)):
        t = PairTarget(ya, yb, torch.tensor([[wa, 1.0 - wa]]).expand(5, 2))
        assert torch.allclose(CrossEntropyLoss(0.1)(lg, t), F.cross_entropy(lg, y, label_smoothing=0.1), rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------ plan properties
def test_plan_depends_on_seed_epoch_rank_and_step_only():
    m = Mix(0.2, 1.0, seed=5)
    a = m.plan(3, 1, 40, H, W)
    b = m.plan(3, 1, 7, H, W)  # another batch size / world size: another number of steps
    for f in ("mode", "box", "lam", "wa", "wb"):
        assert torch.equal(getattr(a, f)[:7], getattr(b, f)), f
        assert torch.equal(getattr(a, f), getattr(m.plan(3, 1, 40, H, W), f)), f  # the same epoch repeats
    assert not torch.equal(a.lam, m.plan(4, 1, 40, H, W).lam)  # two epochs differ
    assert not torch.equal(a.lam, m.plan(3, 0, 40, H, W).lam)  # two ranks differ
    assert not torch.equal(a.lam, Mix(0.2, 1.0, seed=6).plan(3, 1, 40, H, W).lam)
    assert {int(v) for v in a.mode} == {MIXUP, CUTMIX}
    # the rows of a batch do not depend on its size beyond B itself
    t8, w8 = a.rows_for(2, 8)
    t5, w5 = a.rows_for(2, 5)
    assert torch.equal(t8[1:5, 1:], t5[1:, 1:]) and torch.equal(w8[:5], w5)
    assert t5[:, 0].tolist() == [4, 0, 1, 2, 3] and a.rows_for(2, 1)[0][0, 0] == 0
    # the seed is neither the sampler's nor the augmentation's
    assert m.stream_seed(3, 1) not in (5 + 3, Augment(seed=5).stream_seed(3))


def test_plan_modes_weights_and_probabilities():
    n = 400
    both = Mix(0.2, 1.0, prob=0.5, switch_prob=0.25, seed=0).plan(0, 0, n, H, W)
    mixed = (both.mode != NONE).sum().item()
    assert 0.4 * n < mixed < 0.6 * n and 0.15 * mixed < (both.mode == CUTMIX).sum().item() < 0.35 * mixed
    assert bool((both.lam[both.mode == NONE] == 1.0).all())
    assert bool((Mix(0.2, 0.0).plan(0, 0, 50, H, W).mode == MIXUP).all())
    cm = Mix(0.0, 1.0).plan(0, 0, 50, H, W)
    assert bool((cm.mode == CUTMIX).all())
    # lam is adjusted from the clipped area, the weights are each rounded once from float64
    area = ((cm.box[:, 2] - cm.box[:, 0]) * (cm.box[:, 3] - cm.box[:, 1])).double()
    assert torch.equal(cm.lam, 1.0 - area / (H * W))
    assert torch.equal(cm.wa, cm.lam.float()) and torch.equal(cm.wb, (1.0 - cm.lam).float())
    # only mixup blends in the gather: cutmix and unmixed batches carry the weight 1 there
    for plan in (cm, both):
        for s in range(20):
            tab, w = plan.rows_for(s, 4)
            wg = MC.bits_to_f32(tab[:, 5])
            assert bool((wg == (plan.wa[s] if plan.mode[s] == MIXUP else 1.0)).all())
            assert bool((w[:, 0] == plan.wa[s]).all()) and bool((w[:, 1] == plan.wb[s]).all())
    assert not Mix().enabled and Mix(0.2, 1.0).describe() == "mixup0.2+cutmix1"
    for bad in (dict(mixup_alpha=-1.0), dict(cutmix_alpha=float("nan")), dict(mixup_alpha=1.0, prob=1.5),
                dict(cutmix_alpha=1.0, switch_prob=-0.1)):
        with pytest.raises(ValueError):
            Mix(**bad)
    with pytest.raises(ValueError, match="partner"):
        mix_table([0, 3, 1], torch.zeros(3, 4), torch.ones(3))


# ---------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("E", [0.0, 0.1])
def test_cpu_loss_is_cross_entropy_with_probability_targets(E):
    B, C = 6, 10
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(B, C, generator=g, dtype=torch.float64, requires_grad=True)
    ya = torch.randint(0, C, (B,), generator=g)
    yb = ya.roll(1)
    yb[::3] = ya[::3]  # rows with y_a == y_b
    w = torch.tensor([[0.3, 0.7]], dtype=torch.float64).expand(B, 2)
    loss = CrossEntropyLoss(E)(lg, PairTarget(ya, yb, w))
    probs = 0.3 * F.one_hot(ya, C).double() + 0.7 * F.one_hot(yb, C).double()
    want = F.cross_entropy(lg, probs, label_smoothing=E)
    assert torch.equal(loss, want)
    # ... which is the weighted sum of the two smoothed cross-entropies, and the float64 reference
    two = 0.3 * F.cross_entropy(lg, ya, label_smoothing=E) + 0.7 * F.cross_entropy(lg, yb, label_smoothing=E)
    assert abs(loss.item() - two.item()) < 1e-13
    _, ref, dl, _ = MC.pair_xent64(lg.detach(), ya, yb, w, E, 1.0 / B)
    assert abs(loss.item() - ref.item()) < 1e-13
    (gr,) = torch.autograd.grad(loss, lg)
    assert torch.allclose(gr, dl, rtol=0, atol=1e-15)


@pytest.mark.parametrize("B,C", [(3, 10), (5, 65), (5, 1000)])
@pytest.mark.parametrize("E", [0.0, 0.1])
def test_loss_bounds_admit_the_emulated_kernels_and_reject_planted_errors(B, C, E):
    eps, gs = LS.f32(E), LS.f32(1.0 / B)
    for wa in (0.0, 1.0, 0.3):
        lg, ya, yb, w = MC.pair_inputs(B, C, wa)
        loss_ref, dl_ref, bl, bd = MC.pair_bounds(lg, ya, yb, w, eps, gs)
        loss, dl = MC.emulate_pair(lg, ya, yb, w, eps, gs)
        ok_l, r_l = LS.within(loss, loss_ref, bl)
        ok_d, r_d = LS.within(dl, dl_ref, bd)
        assert ok_l and ok_d, (wa, r_l, r_d)
        wrong = ["eps_twice"] if E else []
        wrong += ["swapped", "no_pair"] if wa == 0.3 else []
        for variant in wrong:
            loss, dl = MC.emulate_pair(lg, ya, yb, w, eps, gs, variant)
            assert not (LS.within(loss, loss_ref, bl)[0] and LS.within(dl, dl_ref, bd)[0]), variant
    # lam0 in place of the area-adjusted lam: the weights of a clipped box
    (_, lam) = cutmix_box(0.75, 2, 1, H, W)
    lg, ya, yb, w = MC.pair_inputs(B, C, lam)
    loss_ref, dl_ref, bl, bd = MC.pair_bounds(lg, ya, yb, w, eps, gs)
    w0 = MC.pair_inputs(B, C, 0.75)[3]
    loss, dl = MC.emulate_pair(lg, ya, yb, w0, eps, gs)
    assert not LS.within(dl, dl_ref, bd)[0]


# -------------------------------------------------------------------------------------- pixels
def _own_refs(imgs, rows, aff, resample):
    ref = apply_reference(imgs, rows, aff, resample)
    return ref, MC.norm_error(imgs, rows, aff, resample, ref)


@pytest.mark.parametrize("resample", [False, True])
def test_pixel_bound_admits_the_host_path_and_rejects_planted_errors(resample):
    B = 5
    imgs = AC.images(B, H, W, seed=7)
    rows = (Augment(rrc=True, flip=True, seed=1) if resample else Augment(crop_pad=3, flip=True, seed=1)).plan(0, B, H, W).rows
    rows[:, 4] = torch.tensor([1, 0, 1, 1, 0])
    aff = AC.NEG_AFFINE  # a negative slope: blending before the normalisation shows
    ref, err = _own_refs(imgs, rows, aff, resample)
    n32 = normalized_fp32(imgs, rows, aff, resample)
    lam = 0.3
    wa = float(torch.tensor(lam, dtype=torch.float64).float())
    mref, bound = MC.mixup_bound(ref, ref.roll(1, 0), err, err.roll(1, 0), lam)
    want, _ = mix_reference(ref, torch.zeros(B, dtype=torch.int64), 2, MIXUP, None, lam)
    assert torch.allclose(mref, want, rtol=0, atol=1e-12)
    got = mix_fp32(n32, MC.table(B, (0, 0, 0, 0), wa))
    r = MC.worst_ratio(got, mref, bound)
    print(f"mixup host path, resample={resample}: error / bound = {r:.3f}")
    assert r <= 1.0
    # planted: weights swapped, partner b + 1
    assert MC.worst_ratio(mix_fp32(n32, MC.table(B, (0, 0, 0, 0), 1.0 - wa)), mref, bound) > 1.0
    nxt = (torch.arange(B) + 1) % B
    assert MC.worst_ratio(mix_fp32(n32, MC.table(B, (0, 0, 0, 0), wa, nxt)), mref, bound) > 1.0
    if not resample:
        # blending the uint8 values before the normalisation, rounded to uint8 as an image would be
        u8 = (lam * _raw(imgs, rows) + (1 - lam) * _raw(imgs, rows).roll(1, 0)).round()
        early = (u8 * aff.double()[:, 0] + aff.double()[:, 1]).float().to(torch.bfloat16).float()
        assert MC.worst_ratio(early, mref, bound) > 1.0


def _raw(imgs, rows):
    """The cropped, flipped uint8 values themselves (the affine 1 v + 0), float64."""
    return apply_reference(imgs, rows, torch.tensor([[1.0, 0.0]] * 3), False)


def test_cutmix_copies_pixels_in_output_coordinates():
    """Cutmix and unmixed batches are the augmenting path's own bits of the chosen source; a box
    taken in source coordinates or applied before the flip is not."""
    B = 5
    imgs = AC.images(B, H, W, seed=8)
    rows = Augment(crop_pad=3, flip=True, seed=2).plan(0, B, H, W).rows
    rows[:, 4] = 1  # every image flipped
    aff = AC.IMAGENET_AFFINE
    own = apply_fp32(imgs, rows, aff)
    n32 = normalized_fp32(imgs, rows, aff)
    for name, box in MC.box_cases(H, W):
        tab = MC.table(B, box, 1.0)
        inb = MC.in_box(tab, H, W)[..., None]
        got = mix_fp32(n32, tab)
        assert torch.equal(got, torch.where(inb, own.roll(1, 0), own)), name
        ref, _ = mix_reference(apply_reference(imgs, rows, aff), torch.zeros(B, dtype=torch.int64), 2, CUTMIX, box, 0.5)
        assert torch.equal(got.double(), AC.to_bf16(ref)), name
    box = (2, 3, 9, 8)
    got = mix_fp32(n32, MC.table(B, box, 1.0))
    mirrored = (W - 9, 3, W - 2, 8)  # the same box before the flip / in the flipped source's columns
    assert not torch.equal(got, mix_fp32(n32, MC.table(B, mirrored, 1.0)))


def test_cpu_loader_yields_pair_targets_and_leaves_the_plain_loader_alone():
    n = 37
    imgs, labels = AC.images(n, H, W, seed=5), torch.arange(n) % 10
    aug = Augment(crop_pad=3, flip=True, seed=2)
    norm = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD)
    data = DeviceImages(imgs, labels, "cpu", **norm)
    mix = Mix(0.2, 1.0, seed=2)
    plain = DeviceImageLoader(data, 8, 1, 0, augment=aug)
    mixed = DeviceImageLoader(data, 8, 1, 0, augment=aug, mix=mix)
    assert DeviceImageLoader(data, 8, 1, 0, augment=aug, mix=Mix()).mix is None
    for epoch in (0, 1):
        plain.sampler.set_epoch(epoch)
        mixed.sampler.set_epoch(epoch)
        mp_ = mix.plan(epoch, 0, len(mixed), H, W)
        sizes = []
        for step, ((x, y), (xm, t)) in enumerate(zip(plain, mixed)):
            assert isinstance(t, PairTarget) and torch.equal(t.y_a, y) and torch.equal(t.y_b, y.roll(1))
            assert bool((t.w[:, 0] == mp_.wa[step]).all()) and t.w.shape == (len(y), 2)
            sizes.append(len(y))
            xr = x.roll(1, 0)
            if int(mp_.mode[step]) != MIXUP:  # copies of the augmenting gather's pixels
                x1, y1, x2, y2 = mp_.box[step].tolist()
                want = x.clone()
                want[:, :, y1:y2, x1:x2] = xr[:, :, y1:y2, x1:x2]
                assert torch.equal(xm, want)
            else:
                lam = float(mp_.lam[step])
                assert torch.allclose(xm, lam * x + (1 - lam) * xr, rtol=2.0 ** -7, atol=2.0 ** -7)
        assert sizes == [8, 8, 8, 8, 5]


# ---------------------------------------------------------------------------- CLI and trainer
def _opts(ckdir, **kw):
    from ddp_amd.engine.trainer import TrainOptions

    return TrainOptions(backend="gloo", device="cpu", checkpoint_dir=ckdir, log_every=1, model="resnet18",
                        image_size=32, num_classes=10, dataset_size=32, momentum=0.9, **kw)


def test_option_refusals_and_cli_flags():
    import train_ddp
    from ddp_amd.engine.trainer import TrainOptions, build_mix, check_fused_engine_options, validate_options

    validate_options(_opts("x", mixup_alpha=0.2, cutmix_alpha=1.0, label_smoothing=0.1))
    for bad in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mixup_alpha=0.2, mix_prob=1.5),
                dict(cutmix_alpha=1.0, mix_switch_prob=-0.5), dict(mixup_alpha=float("nan"))):
        with pytest.raises(ValueError, match="mix"):
            validate_options(_opts("x", **bad))
    for flag in (dict(mixup_alpha=0.2), dict(cutmix_alpha=1.0)):
        with pytest.raises(ValueError, match="resnet18"):
            validate_options(TrainOptions(model="simplecnn", **flag))
        with pytest.raises(ValueError, match="fused"):
            check_fused_engine_options(TrainOptions(model="simplecnn", **flag), True)
    assert build_mix(_opts("x")) is None
    assert build_mix(_opts("x", mixup_alpha=0.2, cutmix_alpha=1.0)).describe() == "mixup0.2+cutmix1"
    a = train_ddp.parse_args(["--model", "resnet18", "--mixup_alpha", "0.2", "--cutmix_alpha", "1.0"])
    assert (a.mixup_alpha, a.cutmix_alpha, a.mix_prob, a.mix_switch_prob) == (0.2, 1.0, 1.0, 0.5)
    a = train_ddp.parse_args([])
    assert a.mixup_alpha == 0.0 and a.cutmix_alpha == 0.0
    with pytest.raises(ValueError, match="resnet18"):
        train_ddp.main(["--mixup_alpha", "0.2"])


def _worker(rank, ws, port, ckdir, epochs, kw, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from ddp_amd.engine.trainer import ddp_train

    model = ddp_train(rank, ws, epochs, 8, _opts(ckdir, **kw))
    if rank == 0:
        q.put({n: p.detach().cpu().numpy().copy() for n, p in model.state_dict().items()})


def _train(ckdir, epochs, ws=2, expect_crash=False, **kw):
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), free_port()
    ps = [ctx.Process(target=_worker, args=(r, ws, port, str(ckdir), epochs, kw, q)) for r in range(ws)]
    for p in ps:
        p.start()
    out = None if expect_crash else q.get(timeout=600)
    for p in ps:
        p.join(timeout=600)
    if expect_crash:
        assert [p.exitcode for p in ps] == [17] * ws
    return out


@pytest.mark.slow
def test_two_rank_cpu_crash_and_resume_is_bitwise(tmp_path):
    kw = dict(mixup_alpha=0.2, cutmix_alpha=1.0, label_smoothing=0.1, aug_crop_pad=2, aug_flip=True, normalize=True)
    whole = _train(tmp_path / "a", 2, **kw)
    _train(tmp_path / "b", 2, expect_crash=True, fault=(1, 1, -1), **kw)  # both ranks die inside epoch 1
    assert sorted(os.listdir(tmp_path / "b")) == ["epoch_0.pt"]
    resumed = _train(tmp_path / "b", 2, **kw)
    for n in whole:
        assert whole[n].tobytes() == resumed[n].tobytes(), n
    plain = _train(tmp_path / "c", 2, **{k: v for k, v in kw.items() if k not in ("mixup_alpha", "cutmix_alpha")})
    assert any(whole[n].tobytes() != plain[n].tobytes() for n in whole)
