"""Data layer (reference data.py): MNIST-shaped data, DistributedSampler-exact sharding,
the reference's CPU DataLoader and the HBM-resident device loader."""
from .augment import IMAGENET_MEAN, IMAGENET_STD, AugPlan, Augment, affine_table, apply_fp32, apply_reference
from .imagenet import DeviceImageLoader, DeviceImages, synthetic_imagenet, synthetic_imagenet_test
from .mix import Mix, MixPlan, PairTarget, mix_fp32, mix_reference, mix_table
from .loader import DeviceMNIST, DeviceMNISTLoader, get_dataloader
from .mnist import (MNISTDataset, load_mnist, mnist_available, read_idx, synthetic_mnist,
                    synthetic_mnist_test)
from .sampler import ShardedSampler, epoch_indices, num_samples, steps_per_epoch

__all__ = ["Mix", "MixPlan", "PairTarget", "mix_fp32", "mix_reference", "mix_table", "IMAGENET_MEAN", "IMAGENET_STD", "AugPlan", "Augment", "affine_table", "apply_fp32", "apply_reference",
           "DeviceImageLoader", "DeviceImages", "synthetic_imagenet", "synthetic_imagenet_test", "DeviceMNIST", "DeviceMNISTLoader", "get_dataloader", "MNISTDataset", "load_mnist",
           "mnist_available", "read_idx", "synthetic_mnist", "synthetic_mnist_test", "ShardedSampler", "epoch_indices",
           "num_samples", "steps_per_epoch"]
