"""Synthetic ImageNet-shaped data for ResNet-18 (BASELINE.json config 5).

There is no network for ImageNet here, so the dataset is generated: ``n`` uint8 RGB
images of ``size x size`` (stored NHWC, 150 KB each at 224) with labels in
``[0, num_classes)``.  Each class has its own mean colour and the images carry seeded
per-pixel noise, so a network can fit them and the loss curve means something.

Like the MNIST loader, the set lives in HBM; a batch is a device-side gather that the
``image_gather_nhwc4`` HIP kernel turns straight into the stem's input format: NHWC bf16
with the 3 channels zero-padded to 4, scaled by 1/255 (ToTensor semantics, no
normalisation - like the reference's MNIST pipeline).  On the CPU the same data comes
out as NCHW float for the PyTorch oracle path.  Optionally the gather normalises
(``DeviceImages(mean=, std=)``) and augments (``DeviceImageLoader(augment=)``: random crop
with padding or random resized crop, horizontal flip - ``augment.py``) in the same pass,
through the ``image_gather_aug_nhwc4`` kernel, and mixes each batch with its rolled self
(``DeviceImageLoader(mix=)``: mixup / cutmix - ``mix.py``) through ``image_gather_mix_nhwc4``.
"""
from __future__ import annotations

import torch

from .augment import AugPlan, Augment, affine_table, apply_fp32, normalized_fp32
from .mix import Mix, PairTarget, mix_fp32
from .sampler import ShardedSampler, steps_per_epoch


def synthetic_imagenet(n: int = 2048, size: int = 224, num_classes: int = 1000, seed: int = 0):
    """``(uint8 [n, size, size, 3], int64 [n])`` - class-coloured noisy images."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, num_classes, (n,), generator=g)
    colours = torch.randint(32, 224, (num_classes, 3), generator=g, dtype=torch.int16)
    imgs = torch.empty(n, size, size, 3, dtype=torch.uint8)
    for s in range(0, n, 64):  # bounded temporaries
        e = min(n, s + 64)
        noise = torch.randint(-32, 33, (e - s, size, size, 3), generator=g, dtype=torch.int16)
        imgs[s:e] = (colours[labels[s:e]].view(-1, 1, 1, 3) + noise).clamp_(0, 255).to(torch.uint8)
    return imgs, labels


def synthetic_imagenet_test(n: int, size: int = 224, num_classes: int = 1000, seed: int = 0, n_train: int = 2048):
    """The synthetic held-out split: ``(uint8 [n, size, size, 3], int64 [n])`` in the SAME class
    colours as ``synthetic_imagenet(n_train, size, num_classes, seed)`` (that generator is
    replayed up to its colour draw), labels and noise from a generator of its own - so the
    split is deterministic and no test image repeats a train image."""
    g = torch.Generator().manual_seed(seed)
    torch.randint(0, num_classes, (n_train,), generator=g)  # the train labels' draw
    colours = torch.randint(32, 224, (num_classes, 3), generator=g, dtype=torch.int16)
    gt = torch.Generator().manual_seed(0x7E57 + 1000003 * seed)
    labels = torch.randint(0, num_classes, (n,), generator=gt)
    imgs = torch.empty(n, size, size, 3, dtype=torch.uint8)
    for s in range(0, n, 64):  # bounded temporaries
        e = min(n, s + 64)
        noise = torch.randint(-32, 33, (e - s, size, size, 3), generator=gt, dtype=torch.int16)
        imgs[s:e] = (colours[labels[s:e]].view(-1, 1, 1, 3) + noise).clamp_(0, 255).to(torch.uint8)
    return imgs, labels


class DeviceImages:
    """uint8 NHWC images + int64 labels resident on one device."""

    def __init__(self, images_u8: torch.Tensor, labels: torch.Tensor, device, mean=None, std=None):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
            raise ValueError(f"expected uint8 [N,H,W,3] images, got {images_u8.dtype} {tuple(images_u8.shape)}")
        if labels.shape[0] != images_u8.shape[0]:
            raise ValueError("images and labels differ in length")
        self.device = torch.device(device)
        self.images_u8 = images_u8.contiguous().to(self.device)
        self.labels = labels.to(torch.int64).to(self.device)
        # normalisation is a property of the data set: every gather (train, evaluation) applies it
        self.normalized = mean is not None
        self.affine = affine_table(mean, std)  # float32 [3, 2] on the host (a kernel argument)
        self._identity = {}

    def _identity_plan(self, resample: bool = False) -> AugPlan:
        if resample not in self._identity:
            n, h, w, _ = self.images_u8.shape
            self._identity[resample] = AugPlan.identity(n, h, w, resample).to(self.device)
        return self._identity[resample]

    def __len__(self) -> int:
        return self.images_u8.shape[0]

    def gather(self, idx: torch.Tensor, plan: AugPlan | None = None, mix: torch.Tensor | None = None):
        """GPU: ``(bf16 [B,H,W,4] NHWC4, int64 [B])``; CPU: ``(float32 [B,3,H,W], int64 [B])``.
        ``plan``: the epoch's augmentation table (rows indexed by the data-set index, on this
        device).  With a plan or a normalisation the augmenting kernel runs, and the CPU returns
        the values it stores (bf16-rounded; the integer build bit for bit); with neither, the
        plain gather as before.  ``mix``: the batch's int32 ``[B, 6]`` mixing table
        (``mix.MixPlan.rows_for``, on this device): the mixing kernel runs, every row and its
        partner read through their own rows of ``plan``; the CPU follows the kernel's fp32 order
        (bit for bit where the batch copies pixels: cutmix and unmixed batches of the integer
        build).  The labels returned are the batch's own."""
        y = self.labels.index_select(0, idx)
        if mix is not None:
            return self._gather_mixed(idx, plan, mix), y
        augmented = plan is not None or self.normalized
        if self.device.type == "cuda":
            from .. import native

            n, h, w, _ = self.images_u8.shape
            out = torch.empty(idx.numel(), h, w, 4, dtype=torch.bfloat16, device=self.device)
            if augmented:
                plan = plan if plan is not None else self._identity_plan()
                native.require().image_gather_aug_nhwc4(self.images_u8, idx, plan.rows, self.affine, out,
                                                        plan.resample)
            else:
                native.require().image_gather_nhwc4(self.images_u8, idx, out)
            return out, y
        if augmented:
            plan = plan if plan is not None else self._identity_plan()
            x = apply_fp32(self.images_u8.index_select(0, idx), plan.rows.index_select(0, idx), self.affine,
                           plan.resample)
            return x.permute(0, 3, 1, 2).contiguous(), y
        x = self.images_u8.index_select(0, idx).permute(0, 3, 1, 2).float().div_(255.0)
        return x, y


    def _gather_mixed(self, idx, plan, mix):
        plan = plan if plan is not None else self._identity_plan()
        if self.device.type == "cuda":
            from .. import native

            n, h, w, _ = self.images_u8.shape
            out = torch.empty(idx.numel(), h, w, 4, dtype=torch.bfloat16, device=self.device)
            native.require().image_gather_mix_nhwc4(self.images_u8, idx, plan.rows, self.affine, mix, out,
                                                    plan.resample)
            return out
        n32 = normalized_fp32(self.images_u8.index_select(0, idx), plan.rows.index_select(0, idx), self.affine,
                              plan.resample)
        return mix_fp32(n32, mix).permute(0, 3, 1, 2).contiguous()


class DeviceImageLoader:
    """The rank's ``DistributedSampler``-exact batches out of device memory (ragged last
    batch, drop_last=False), one index upload per epoch.  With ``mix`` a batch is
    ``(images, PairTarget)``: the mixed images and the two labels with their weights."""

    def __init__(self, data: DeviceImages, batch_size: int, world_size: int, rank: int,
                 shuffle: bool = True, seed: int = 0, augment: Augment | None = None, mix: Mix | None = None):
        self.data, self.batch_size, self.augment = data, int(batch_size), augment
        self.mix = mix if mix is not None and mix.enabled else None
        self.sampler = ShardedSampler(len(data), world_size, rank, shuffle=shuffle, seed=seed)

    def __len__(self) -> int:
        return steps_per_epoch(len(self.data), self.sampler.num_replicas, self.batch_size)

    def __iter__(self):
        idx = self.sampler.indices().to(self.data.device, non_blocking=False)
        plan = None
        if self.augment is not None:  # the epoch's table, uploaded once with the index list
            n, h, w, _ = self.data.images_u8.shape
            plan = self.augment.plan(self.sampler.epoch, n, h, w).to(self.data.device)
        if self.mix is None:
            for s in range(0, idx.numel(), self.batch_size):
                yield self.data.gather(idx[s:s + self.batch_size], plan)
            return
        n, h, w, _ = self.data.images_u8.shape
        mplan = self.mix.plan(self.sampler.epoch, self.sampler.rank, len(self), h, w)
        for step, s in enumerate(range(0, idx.numel(), self.batch_size)):
            bidx = idx[s:s + self.batch_size]
            table, wts = mplan.rows_for(step, bidx.numel())  # validated on the host, then uploaded
            x, y = self.data.gather(bidx, plan, table.to(self.data.device))
            yield x, PairTarget(y, y.index_select(0, table[:, 0].to(torch.int64).to(y.device)),
                                wts.to(self.data.device))
