"""Per-rank training entry point - the reference's ``ddp_train`` (train_ddp.py:17-212).

Same phases, same log lines, same checkpoint/resume contract,
with the reference's bugs fixed and the hot loop replaced:

* GPU (default): the native fused step engine - 2 HIP kernels per step on one GPU
  (fuse level 3), plus the light fc weight-gradient kernel and one direct-xGMI (or RCCL)
  all-reduce per gradient bucket on several, hipGraph-replayed, dataset resident in HBM;
* GPU ``--engine module``: the module path (HIP autograd Functions + our DDP with
  the native C++ reducer) - the reference's loop shape, kernel-for-kernel on HIP;
* GPU with ``--backend gloo --device gpu``: the same GPU paths with a gloo control plane
  and the direct xGMI data plane - several ranks may share one GPU, which rehearses the
  multi-GPU trainer (checkpoint / resume, bucket all-reduces) on a single device;
* CPU: gloo + the reference's loop over a DataLoader (BASELINE config 1).

``model="resnet18"`` (BASELINE config 5) trains torchvision-layout ResNet-18 on
synthetic ImageNet-shaped data through the module path (GPU: the HIP ResNet Functions,
our DDP and the native reducer, optionally the whole step in one hipGraph; CPU: the
PyTorch oracle), with the same launcher, logging, checkpoint and resume contract.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
import time

import torch
import torch.distributed as dist

from ..data import (DeviceImageLoader, DeviceImages, DeviceMNIST, DeviceMNISTLoader, get_dataloader,
                    load_mnist, synthetic_imagenet, synthetic_imagenet_test)
from ..models import SimpleCNN, resnet18
from ..models.layers import buffer_space, flat_space
from ..ops import CrossEntropyLoss, FusedAdamW, FusedLARS, FusedSGD
from ..parallel import DistributedDataParallel as DDP
from ..parallel import cleanup, local_rank, native_comm, setup
from ..utils.checkpoint import resume, resume_ema, save_checkpoint


@dataclasses.dataclass
class TrainOptions:
    lr: float = 0.01
    momentum: float = 0.0
    weight_decay: float = 0.0
    backend: str | None = None        # rccl|nccl|gloo (default: rccl on GPU, gloo on CPU)
    device: str | None = None         # auto|gpu|cpu: "gpu" fails loudly without a usable HIP device
    engine: str = "fused"             # fused | module   (GPU only)
    data: str = "auto"                # auto | mnist | synthetic
    data_root: str = "./data"
    checkpoint_dir: str = "./checkpoints"
    save: bool = True
    seed: int | None = 0
    log_every: int = 100
    graph_steps: int = 100
    bucket_cap_mb: float = 25.0
    num_workers: int = 2
    max_steps: int | None = None      # stop each epoch early (smoke tests)
    metrics_json: str | None = None   # append per-epoch throughput records here
    fault: tuple | None = None        # (epoch, step, rank|-1): simulate a crash there (resume tests)
    fuse_level: int | None = None     # fused engine fusion level (None: engine default)
    comm: str = "auto"                # fused engine bucket all-reduce: auto/xgmi (direct kernel) | rccl
    # fused engine at world size 1: run the multi-GPU step chain anyway (fc_bwd on the forked
    # branch, the bucket all-reduces of the 8-rank plan on the --comm plane, the start-up chain
    # check) - the production ws > 1 chain, rehearsed (and pinned by tests) on one GPU
    force_allreduce: bool = False
    grad_accum: int = 1               # micro-batches per optimizer step (module/CPU path)
    global_loss: bool = False         # log the all-reduced mean loss (module/CPU path, bug B14)
    pg_timeout_s: float | None = None
    model: str = "simplecnn"          # simplecnn | resnet18 (BASELINE config 5)
    image_size: int = 224             # resnet18: synthetic image side
    num_classes: int = 1000           # resnet18
    dataset_size: int = 2048          # resnet18: synthetic images resident per rank
    graph_module: bool = False        # module path on GPU: capture each step in a hipGraph
    dtype: str = "bf16"               # GPU compute precision: bf16 | fp32 (exact fp32 MFMA, reference precision)
    verify_replicas: bool = False     # after every epoch: all ranks' parameters (+ momentum) bitwise equal, or raise
    stall: tuple | None = None        # (epoch, rank, seconds): that rank sleeps before the epoch's first step
    eval_every: int = 0               # evaluate the held-out split after every Nth epoch (0: never)
    eval_batch_size: int = 1000       # images per evaluation launch / forward
    eval_only: bool = False           # resume from the newest checkpoint, evaluate, exit
    eval_size: int = 0                # resnet18: images of the synthetic held-out split (0: none)
    clip_grad_norm: float = 0.0       # global-norm gradient clipping inside opt.step() (0: off; module/CPU path)
    lr_schedule: str = "none"         # none | cosine | linear | step, per optimizer step (module/CPU path)
    warmup_steps: int = 0             # linear warm-up from 0.01 * lr over the first N optimizer steps
    lr_min: float = 0.0               # cosine / linear: the rate the decay ends at
    lr_step_epochs: int = 0           # step: multiply the rate by lr_gamma every N epochs
    lr_gamma: float = 0.1
    optimizer: str = "sgd"            # sgd | adamw | lars (adamw, lars: module/CPU path)
    beta1: float = 0.9                # adamw
    beta2: float = 0.999              # adamw
    adam_eps: float = 1e-8            # adamw
    trust_coef: float = 1e-3          # lars: the trust ratio's coefficient
    lars_eps: float = 1e-8            # lars: the trust ratio denominator's epsilon
    lars_exclude: str = "1d"          # lars: 1d (BatchNorm scales, biases: ratio 1, no decay) | none
    ema_decay: float = 0.0            # weight EMA updated by every optimizer step (0: off; module/CPU path)
    ema_warmup: bool = False          # decay_k = min(ema_decay, (1 + k) / (10 + k)) for update k
    eval_ema: bool = False            # every evaluation also evaluates the averaged weights
    label_smoothing: float = 0.0      # training loss target (1 - e) onehot + e / C, torch's (0: off; module/CPU path)
    normalize: bool = False           # resnet18: ImageNet mean/std normalisation in every gather (train and eval)
    aug_crop_pad: int = 0             # resnet18: random crop with P pixels of black padding (0: off)
    aug_rrc: bool = False             # resnet18: random resized crop (ratio 3/4..4/3), bilinear
    aug_scale_min: float = 0.08       # aug_rrc: the smallest area share of the box
    aug_flip: bool = False            # resnet18: horizontal flip, p = 0.5, after the crop
    mixup_alpha: float = 0.0          # resnet18: mixup with lam ~ Beta(a, a) per batch, in the gather (0: off)
    cutmix_alpha: float = 0.0         # resnet18: cutmix with lam0 ~ Beta(a, a) per batch, in the gather (0: off)
    mix_prob: float = 1.0             # probability that a batch is mixed at all
    mix_switch_prob: float = 0.5      # with both alphas: probability that a mixed batch is a cutmix batch


def validate_options(opts: TrainOptions):
    """Option combinations that cannot run (checked by the CLI before any process starts, and
    by every rank)."""
    if opts.eval_every < 0 or opts.eval_batch_size < 1:
        raise ValueError("--eval_every must be >= 0 and --eval_batch_size >= 1")
    if opts.eval_size < 0:
        raise ValueError("--eval_size must be >= 0")
    if opts.model == "resnet18" and (opts.eval_every or opts.eval_only) and not opts.eval_size:
        raise ValueError("--eval_every / --eval_only evaluate SimpleCNN on the MNIST test split; the synthetic "
                         "ImageNet set of --model resnet18 has no held-out split unless --eval_size N builds one")
    if opts.model != "resnet18" and opts.eval_size:
        raise ValueError("--eval_size sizes the synthetic held-out split of --model resnet18; simplecnn's "
                         "split is the MNIST test set")
    if opts.clip_grad_norm < 0:
        raise ValueError("--clip_grad_norm must be >= 0 (0 = off)")
    if opts.lr_schedule not in ("none", "cosine", "linear", "step"):
        raise ValueError(f"--lr_schedule must be none, cosine, linear or step, got {opts.lr_schedule!r}")
    if opts.warmup_steps < 0:
        raise ValueError("--warmup_steps must be >= 0")
    if opts.lr_schedule == "step" and opts.lr_step_epochs < 1:
        raise ValueError("--lr_schedule step needs --lr_step_epochs N >= 1")
    if opts.optimizer not in ("sgd", "adamw", "lars"):
        raise ValueError(f"--optimizer must be sgd, adamw or lars, got {opts.optimizer!r}")
    if opts.optimizer == "lars":
        if not opts.trust_coef > 0 or opts.lars_eps < 0:
            raise ValueError("--trust_coef must be positive and --lars_eps >= 0")
        if opts.lars_exclude not in ("1d", "none"):
            raise ValueError(f"--lars_exclude must be 1d or none, got {opts.lars_exclude!r}")
    if not 0.0 <= opts.ema_decay < 1.0:
        raise ValueError("--ema_decay must lie in [0, 1) (0 = off)")
    if (opts.eval_ema or opts.ema_warmup) and not opts.ema_decay:
        raise ValueError("--eval_ema / --ema_warmup need a weight EMA: set --ema_decay D")
    if not 0.0 <= opts.label_smoothing <= 1.0:
        raise ValueError("--label_smoothing must lie in [0, 1] (0 = off)")
    if opts.aug_crop_pad < 0:
        raise ValueError("--aug_crop_pad must be >= 0 (0 = off)")
    if opts.aug_crop_pad and opts.aug_rrc:
        raise ValueError("--aug_crop_pad and --aug_rrc are two crop modes: choose one")
    if opts.aug_crop_pad >= opts.image_size and opts.model == "resnet18":
        raise ValueError(f"--aug_crop_pad must be smaller than --image_size {opts.image_size}")
    if not 0.0 < opts.aug_scale_min <= 1.0:
        raise ValueError("--aug_scale_min must lie in (0, 1]")
    if opts.model != "resnet18" and uses_augment(opts):
        raise ValueError("--normalize / --aug_crop_pad / --aug_rrc / --aug_flip run inside the image gather of "
                         "--model resnet18; simplecnn's MNIST loaders and the fused engine's in-kernel gather "
                         "have no augmenting build")
    if not (opts.mixup_alpha >= 0.0 and opts.cutmix_alpha >= 0.0):
        raise ValueError("--mixup_alpha and --cutmix_alpha must be >= 0 (0 = off)")
    if not (0.0 <= opts.mix_prob <= 1.0 and 0.0 <= opts.mix_switch_prob <= 1.0):
        raise ValueError("--mix_prob and --mix_switch_prob must lie in [0, 1]")
    if opts.model != "resnet18" and uses_mix(opts):
        raise ValueError("--mixup_alpha / --cutmix_alpha mix batches inside the image gather of --model resnet18 "
                         "and train against pair targets; simplecnn's MNIST loaders have no mixing gather and "
                         "the fused engine computes its loss from the data set's own labels")
    if opts.optimizer == "adamw" and opts.momentum != 0:
        raise ValueError("--momentum is SGD's; --optimizer adamw takes --beta1 / --beta2 / --adam_eps")
    if (opts.device or "").lower() == "gpu":  # the fused engine is certain: refuse before any process starts
        check_fused_engine_options(opts, opts.engine == "fused" and opts.model == "simplecnn")


def check_fused_engine_options(opts: TrainOptions, fused: bool):
    """Options the fused SimpleCNN engine cannot honour (``fused``: this run uses it)."""
    if fused and (opts.grad_accum != 1 or opts.global_loss):
        raise ValueError("--grad_accum / --global_loss need the module path (--engine module) "
                         "or the CPU path; the fused engine runs one micro-batch per step")
    if fused and opts.clip_grad_norm:
        raise ValueError("--clip_grad_norm needs the module path (--engine module) or the CPU path; the "
                         "fused engine applies SGD inside the kernels that finish each gradient, before "
                         "the global norm exists")
    if fused and uses_lr_schedule(opts):
        raise ValueError("--lr_schedule / --warmup_steps need the module path (--engine module) or the CPU "
                         "path; the fused engine bakes the learning rate into its kernels' arguments and "
                         "into its captured step graphs")
    if fused and opts.ema_decay:
        raise ValueError("--ema_decay needs the module path (--engine module) or the CPU path; the fused "
                         "engine applies SGD inside the kernels that finish each gradient and its captured "
                         "step graphs hold no averaging pass")
    if fused and opts.label_smoothing:
        raise ValueError("--label_smoothing needs the module path (--engine module) or the CPU path; the "
                         "fused engine computes its loss inside the forward and fc_bwd kernels, which have "
                         "no smoothed build")
    if fused and uses_mix(opts):
        raise ValueError("--mixup_alpha / --cutmix_alpha need --model resnet18 (module path); the fused "
                         "engine gathers its batch inside the forward kernel and reads the data set's own "
                         "labels, which have no pair build")
    if fused and opts.optimizer == "lars":
        raise ValueError("--optimizer lars needs the module path (--engine module) or the CPU path; the "
                         "fused engine applies SGD inside the kernels that finish each gradient, before "
                         "any tensor's gradient norm exists")
    if fused and opts.optimizer != "sgd":
        raise ValueError("--optimizer adamw needs the module path (--engine module) or the CPU path; the "
                         "fused engine applies SGD inside the kernels that finish each gradient and keeps "
                         "no second-moment state")


def uses_lr_schedule(opts: TrainOptions) -> bool:
    return opts.lr_schedule != "none" or opts.warmup_steps > 0


def uses_augment(opts: TrainOptions) -> bool:
    return bool(opts.normalize or opts.aug_crop_pad or opts.aug_rrc or opts.aug_flip)


def uses_mix(opts: TrainOptions) -> bool:
    return bool(opts.mixup_alpha or opts.cutmix_alpha)


def build_mix(opts: TrainOptions):
    """The run's Mix from the flags (None: both alphas 0) - a pure function of the flags and the
    seed, so a resumed run redraws the same records."""
    if not uses_mix(opts):
        return None
    from ..data.mix import Mix

    return Mix(opts.mixup_alpha, opts.cutmix_alpha, prob=opts.mix_prob, switch_prob=opts.mix_switch_prob,
               seed=opts.seed or 0)


def build_augment(opts: TrainOptions):
    """The run's Augment from the flags (None: no crop and no flip) - a pure function of the
    flags and the seed, so every rank and every resumed run draws the same tables."""
    if not (opts.aug_crop_pad or opts.aug_rrc or opts.aug_flip):
        return None
    from ..data.augment import Augment

    return Augment(crop_pad=opts.aug_crop_pad, rrc=opts.aug_rrc, scale=(opts.aug_scale_min, 1.0),
                   flip=opts.aug_flip, seed=opts.seed or 0)


def augment_tag(opts: TrainOptions) -> str:
    """``rrc+flip+norm``-style summary for the metrics records ('' when everything is off)."""
    aug = build_augment(opts)
    return "+".join(([aug.describe()] if aug is not None else []) + (["norm"] if opts.normalize else []))


def optimizer_steps_per_epoch(n_batches: int, grad_accum: int = 1, max_steps: int | None = None) -> int:
    """Optimizer steps of one epoch on a rank: every ``grad_accum`` batches plus the ragged
    flush (``max_steps`` caps the epoch's batches, as _run_module_epoch does)."""
    if max_steps is not None:
        n_batches = min(n_batches, max_steps)
    return -(-n_batches // grad_accum)


def build_lr_schedule(opts: TrainOptions, epochs: int, per_epoch: int):
    """The run's LRSchedule from the flags, or None for a constant rate (then FusedSGD takes
    ``lr`` by value, as before).  A pure function of the flags: every rank builds the same table."""
    if not uses_lr_schedule(opts):
        return None
    from ..ops.lr_schedule import LRSchedule

    return LRSchedule(opts.lr, max(1, epochs * per_epoch), opts.lr_schedule, warmup_steps=opts.warmup_steps,
                      lr_min=opts.lr_min, step_size=opts.lr_step_epochs * per_epoch, gamma=opts.lr_gamma)


def ddp_train(rank: int, world_size: int, epochs: int, batch_size: int,
              opts: TrainOptions | None = None):
    opts = opts or TrainOptions()
    validate_options(opts)
    backend = setup(rank=rank, world_size=world_size, backend=opts.backend,
                    timeout_s=opts.pg_timeout_s, device=opts.device)
    # RCCL means the GPU; gloo means the GPU only when it was asked for explicitly (a gloo
    # control plane over GPU tensors + the direct xGMI data plane: same-GPU rehearsals)
    want = (opts.device or os.environ.get("DDP_AMD_DEVICE") or "auto").lower()
    on_gpu = backend == "nccl" or (want == "gpu" and torch.cuda.is_available())
    device = torch.device("cuda", local_rank(rank)) if on_gpu else torch.device("cpu")
    if on_gpu:
        torch.cuda.set_device(device)
    print(f"Rank {rank} initialized", flush=True)
    if opts.grad_accum < 1:
        raise ValueError("--grad_accum must be >= 1")

    if opts.seed is not None:
        torch.manual_seed(opts.seed)  # B15: reproducible init (rank 0's weights win anyway)
    if opts.model == "resnet18":
        if on_gpu and opts.dtype != "bf16":
            raise ValueError("resnet18 on the GPU runs bf16 MFMA kernels only (--dtype bf16)")
        model = resnet18(num_classes=opts.num_classes).to(device)
        if on_gpu and opts.engine == "fused" and rank == 0:
            print("Rank 0: resnet18 runs on the module path (the fused engine is SimpleCNN's)", flush=True)
    elif opts.model == "simplecnn":
        if opts.dtype not in ("bf16", "fp32"):
            raise ValueError(f"--dtype must be bf16 or fp32, got {opts.dtype!r}")
        model = SimpleCNN(compute_dtype=torch.float32 if opts.dtype == "fp32" else torch.bfloat16).to(device)
    else:
        raise ValueError(f"unknown model {opts.model!r}")
    fused = on_gpu and opts.engine == "fused" and opts.model == "simplecnn"
    check_fused_engine_options(opts, fused)
    if fused:
        fs = flat_space(model)

        _verify_and_broadcast(fs, model, world_size)
        ddp_model = model
    else:
        ddp_model = DDP(model, bucket_cap_mb=opts.bucket_cap_mb, comm=module_comm(opts.comm))
        fs = ddp_model.fs
    print(f"Rank {rank} model wrapped in DDP", flush=True)

    if opts.model == "resnet18":
        from ..data.augment import IMAGENET_MEAN, IMAGENET_STD

        norm = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD) if opts.normalize else {}
        imgs, labels = synthetic_imagenet(opts.dataset_size, opts.image_size, opts.num_classes)
        loader = DeviceImageLoader(DeviceImages(imgs, labels, device, **norm), batch_size, world_size, rank,
                                   augment=build_augment(opts), mix=build_mix(opts))
        sampler = loader.sampler
    elif on_gpu:
        imgs, labels, src = load_mnist(opts.data_root, opts.data)
        ddata = DeviceMNIST(imgs, labels, device, src)
        loader = DeviceMNISTLoader(ddata, batch_size, world_size, rank)
        sampler = loader.sampler
    else:
        loader, sampler = get_dataloader(batch_size, world_size, rank, root=opts.data_root,
                                         source=opts.data, num_workers=opts.num_workers)
    edata = None
    if (opts.eval_every or opts.eval_only) and opts.model == "resnet18":
        timgs, tlabels = synthetic_imagenet_test(opts.eval_size, opts.image_size, opts.num_classes,
                                                 n_train=opts.dataset_size)
        edata, tsrc = DeviceImages(timgs, tlabels, device, **norm), "synthetic"  # evaluation never augments
        if rank == 0:
            print(f"Rank {rank}: Eval split: {tsrc} ({len(edata)} images)", flush=True)
    elif opts.eval_every or opts.eval_only:
        timgs, tlabels, tsrc = load_mnist(opts.data_root, opts.data, split="test")
        edata = DeviceMNIST(timgs, tlabels, device, tsrc)
        if rank == 0:
            print(f"Rank {rank}: Eval split: {tsrc} ({len(edata)} images)", flush=True)
    print(f"Rank {rank}: Dataloader ready", flush=True)
    # the training loss only: evaluation keeps reporting the plain cross-entropy, so evaluation
    # losses stay comparable between runs with different --label_smoothing
    loss_fn = CrossEntropyLoss(label_smoothing=opts.label_smoothing)
    # clipping lives in opt.step(): with --grad_accum only the boundary step clips, and under
    # DDP the norm is of the all-reduced gradient (the same bits, so the same coefficient, on every rank)
    # the schedule is indexed by the global optimizer step: a table every rank builds alike from the
    # flags (no schedule object with the default flags: the by-value sgd_kernel runs)
    per_epoch = optimizer_steps_per_epoch(len(loader), opts.grad_accum, opts.max_steps)
    if opts.optimizer == "adamw":
        opt = FusedAdamW(model, lr=opts.lr, betas=(opts.beta1, opts.beta2), eps=opts.adam_eps,
                         weight_decay=opts.weight_decay, max_grad_norm=opts.clip_grad_norm or None,
                         lr_schedule=build_lr_schedule(opts, epochs, per_epoch))
    elif opts.optimizer == "lars":
        opt = FusedLARS(model, lr=opts.lr, momentum=opts.momentum, weight_decay=opts.weight_decay,
                        trust_coef=opts.trust_coef, eps=opts.lars_eps,
                        exclude=None if opts.lars_exclude == "none" else "1d",
                        max_grad_norm=opts.clip_grad_norm or None,
                        lr_schedule=build_lr_schedule(opts, epochs, per_epoch))
    else:
        opt = FusedSGD(model, lr=opts.lr, momentum=opts.momentum, weight_decay=opts.weight_decay,
                       max_grad_norm=opts.clip_grad_norm or None,
                       lr_schedule=build_lr_schedule(opts, epochs, per_epoch))
    model.train()
    print(f"Rank {rank}: Loss and Optimizer ready", flush=True)

    start_epoch, path = resume(model, opt, opts.checkpoint_dir, rank, world_size,
                               device=device, flat=fs)
    if path is None:
        print(f"Rank {rank}: No checkpoint found, starting from scratch.", flush=True)
    elif rank == 0:
        print(f"Rank {rank}: Resumed from {path}, starting at epoch {start_epoch}", flush=True)
    if path is not None and opts.optimizer == "adamw":
        # the Adam step is optimizer state: it came with the checkpoint, and is the schedule's index
        if opt.schedule_step() != start_epoch * per_epoch:
            print(f"Rank {rank}: WARNING: the checkpoint's optimizer step {opt.schedule_step()} is not "
                  f"{start_epoch * per_epoch}, the step epoch {start_epoch} starts at in this run: the schedule "
                  "flags, --epochs, --batch_size, --grad_accum, --max_steps and the world size must match "
                  "the run that wrote the checkpoint", flush=True)
    elif path is not None and opt.lr_schedule is not None:
        opt.set_schedule_step(start_epoch * per_epoch)  # the schedule is a function of the step index alone
        if opt.loaded_lr is not None and opt.loaded_lr != opt.current_lr():  # (rank 0: it read the file)
            print(f"Rank {rank}: WARNING: the checkpoint's lr {opt.loaded_lr!r} is not this schedule's rate "
                  f"{opt.current_lr()!r} at step {start_epoch * per_epoch}: the schedule flags, --epochs, "
                  "--batch_size, --grad_accum, --max_steps and the world size must match the run that "
                  "wrote the checkpoint", flush=True)

    # the EMA starts from the parameters every rank now holds alike (loaded, or rank 0's through
    # DDP's broadcast) and is a deterministic function of them: it needs no communication
    ema = None
    if opts.ema_decay:
        from ..ops.ema import WeightEMA

        ema = WeightEMA(model, decay=opts.ema_decay, warmup=opts.ema_warmup)
        if path is not None and not resume_ema(ema, opts.checkpoint_dir, rank, world_size, device=device) \
                and rank == 0:
            print(f"Rank {rank}: WARNING: the checkpoint holds no weight EMA: the average restarts from the "
                  "loaded parameters", flush=True)
        opt.attach_ema(ema)

    if opts.eval_only:
        if path is None:
            raise FileNotFoundError(f"--eval_only: no checkpoint under {opts.checkpoint_dir!r}")
        # a bare model's parameters: the fused kernel's operands are built from them
        res = run_eval(model, None, edata, device, opts, rank, world_size, fused)
        _log_eval(rank, start_epoch - 1, res)
        if opts.eval_ema:
            with ema.applied():
                res = run_eval(model, None, edata, device, opts, rank, world_size, fused)
            _log_eval(rank, start_epoch - 1, res, tag="Eval EMA")
        cleanup()
        return model

    engine = None
    if fused:
        from .fused_step import EngineOptions, FusedSimpleCNNEngine

        comm = native_comm() if world_size > 1 and dist.get_backend() == "nccl" else None
        force = bool(opts.force_allreduce) and world_size == 1
        if force and comm is None and opts.comm == "rccl" and dist.get_backend() == "nccl":
            comm = native_comm()
        eo = EngineOptions(graph_steps=opts.graph_steps, bucket_cap_mb=opts.bucket_cap_mb,
                           comm=opts.comm, dtype=opts.dtype, force_allreduce=force,
                           plan_world=8 if force else None)
        if opts.fuse_level is not None:
            eo.fuse_level = opts.fuse_level
        engine = FusedSimpleCNNEngine(model, opt, ddata, batch_size, world_size, rank, comm, eo)
        engine.refresh()
        if world_size > 1 or force:
            # the production chain must give the conservative chain's bits across the real
            # peers before training commits to it (VERDICT r3 #3a); else every rank downgrades
            kept = engine.verify_chain()
            if rank == 0:
                print(f"Rank {rank}: start-up chain check "
                      f"{'passed' if kept else 'FAILED -> conservative chain'} ({engine.chain_check})", flush=True)

    for epoch in range(start_epoch, epochs):
        sampler.set_epoch(epoch)
        print(f"Rank {rank}: Starting epoch {epoch}", flush=True)
        t0 = time.perf_counter()

        def log(batch_idx, loss_value):
            if rank == 0:
                print(f"Epoch {epoch} | Batch {batch_idx} | Loss: {loss_value:.4f}", flush=True)

        fault_step = _fault_step(opts.fault, epoch, rank)
        if opts.stall and int(opts.stall[0]) == epoch and int(opts.stall[1]) == rank:
            print(f"Rank {rank}: injected stall of {float(opts.stall[2]):g} s before epoch {epoch}", flush=True)
            time.sleep(float(opts.stall[2]))  # a slow rank: the peers' all-reduces wait for it
        if fused:
            nsteps = engine.run_epoch(epoch, on_loss=log, log_every=opts.log_every,
                                      max_steps=fault_step if fault_step is not None else opts.max_steps)
            engine.synchronize()
        else:
            nsteps = _run_module_epoch(ddp_model, loader, loss_fn, opt, device, log,
                                       opts.log_every,
                                       fault_step if fault_step is not None else opts.max_steps,
                                       opts.grad_accum, opts.global_loss,
                                       graph=on_gpu and opts.graph_module)
        if fault_step is not None:
            _inject_fault(rank, epoch, nsteps)
        if on_gpu:
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ev = ev_ema = None
        if opts.eval_every and (epoch + 1) % opts.eval_every == 0:
            ev = run_eval(model, engine, edata, device, opts, rank, world_size, fused)
            _log_eval(rank, epoch, ev)
            if opts.eval_ema:
                with ema.applied():
                    ev_ema = run_eval(model, engine, edata, device, opts, rank, world_size, fused)
                _log_eval(rank, epoch, ev_ema, tag="Eval EMA")
        _record_metrics(opts, rank, world_size, epoch, nsteps, batch_size, dt,
                        samples_processed(nsteps, batch_size, len(sampler)), ev, ev_ema=ev_ema,
                        ema_updates=ema.num_updates() if opts.metrics_json and rank == 0 and ema is not None
                        else None,
                        clip=opt.grad_clip_stats() if opts.metrics_json and rank == 0 else None,
                        lr=opt.current_lr() if opts.metrics_json and rank == 0 and opt.lr_schedule is not None
                        else None,
                        trust=opt.trust_stats() if opts.metrics_json and rank == 0 and opts.optimizer == "lars"
                        else None)

        if opts.verify_replicas and world_size > 1:
            verify_replicas(fs, opt, rank, world_size, epoch)
        if rank == 0 and opts.save:
            save_checkpoint(opts.checkpoint_dir, epoch, model, opt)
        if world_size > 1:
            dist.barrier()  # B13: nobody races past a half-written checkpoint
    cleanup()
    return model


def run_eval(model, engine, edata, device, opts, rank: int, world_size: int, fused: bool):
    """This rank's shard of the held-out split (:func:`eval_shard`: every image on exactly one
    rank), then the totals over all ranks.  Fused GPU path: the inference kernel (on the
    engine's stream with the engine's operands, or built from the bare model's parameters);
    module path and CPU: the model's forward under ``no_grad``.  Collective."""
    from .evaluation import all_reduce_result, eval_shard, evaluate, evaluate_resnet

    idx = eval_shard(len(edata), world_size, rank)
    if opts.model == "resnet18":  # GPU: the fused conv + BatchNorm inference path; CPU: the module forward
        with _rank0_buffers(model, world_size):
            res = evaluate_resnet(model, edata, device, opts.eval_batch_size, idx, engine="fused")
    elif engine is not None:
        res = engine.evaluate(edata, opts.eval_batch_size, idx)
    else:
        res = evaluate(model, edata, device, opts.dtype, opts.eval_batch_size, idx,
                       engine="fused" if fused else "module")
    return all_reduce_result(res)


@contextlib.contextmanager
def _rank0_buffers(model, world_size: int):
    """Evaluate with rank 0's BatchNorm running statistics on every rank - the ones DDP
    broadcasts before each forward and the ones the checkpoint holds (a rank's own drift from
    them after its last step) - so the totals do not depend on the sharding.  This rank's own
    buffers are put back afterwards, bit for bit: evaluation leaves no trace.  Collective."""
    bs = buffer_space(model) if world_size > 1 else None
    if bs is None:
        yield
        return
    flats = bs.flat_list()
    saved = [t.clone() for t in flats]
    staged = dist.get_backend() != "nccl"  # gloo control plane: collectives on CPU tensors
    with torch.no_grad():
        for t in flats:
            if staged and t.is_cuda:
                c = t.cpu()
                dist.broadcast(c, src=0)
                t.copy_(c)
            else:
                dist.broadcast(t, src=0)
    try:
        yield
    finally:
        with torch.no_grad():
            for t, s in zip(flats, saved):
                t.copy_(s)


def _log_eval(rank: int, epoch: int, res, tag: str = "Eval"):
    if rank == 0:
        top5 = "" if res.correct5 is None else f" | Top-5: {100.0 * res.top5:.2f}% ({res.correct5}/{res.count})"
        print(f"Epoch {epoch} | {tag} | Loss: {res.mean_loss:.4f} | Accuracy: {100.0 * res.accuracy:.2f}% "
              f"({res.correct}/{res.count}){top5}", flush=True)


def module_comm(comm: str) -> str:
    """The module path's data plane for the trainer's ``--comm`` (the engine's plan names):
    rccl -> RCCL, xgmi / xgmi1 / xgmi2 / tune -> the direct xGMI kernels, auto -> DDP's own
    choice (RCCL under nccl, xGMI under a gloo control plane)."""
    if comm in ("auto", "rccl"):
        return comm
    if comm in ("xgmi", "xgmi1", "xgmi2", "tune"):
        return "xgmi"
    raise ValueError(f"unknown comm {comm!r}")


def replica_digest(fs, opt) -> str:
    """SHA-1 of this rank's flat parameters, every optimizer state buffer (SGD: momentum;
    AdamW: both moments) and, with an attached weight EMA, its buffer and update count: bitwise
    replica identity."""
    import hashlib

    h = hashlib.sha1(fs.params.detach().cpu().numpy().tobytes())
    for buf in opt.state_buffers().values():
        if buf is not None:
            h.update(buf.detach().cpu().numpy().tobytes())
    if getattr(opt, "ema", None) is not None:
        h.update(ema_digest(opt.ema).encode())
    return h.hexdigest()


def ema_digest(ema) -> str:
    """SHA-1 of a WeightEMA's flat buffer and update count."""
    import hashlib

    h = hashlib.sha1(ema.params.detach().cpu().numpy().tobytes())
    h.update(str(ema.num_updates()).encode())
    return h.hexdigest()


def verify_replicas(fs, opt, rank: int, world_size: int, epoch: int):
    """DDP's invariant, checked: every rank holds bitwise the same parameters and optimizer
    state (a divergence would mean a broken all-reduce or a non-deterministic kernel)."""
    import hashlib

    d = replica_digest(fs, opt)
    allg = [None] * world_size
    dist.all_gather_object(allg, d)
    if any(x != allg[0] for x in allg):
        # which tensors differ (and by how much), for the error message
        per = {n: hashlib.sha1(fs.view(fs.params, n).detach().cpu().numpy().tobytes()).hexdigest()
               for n in fs.names}
        mine = fs.params.detach().cpu()
        allp, allpar = [None] * world_size, [None] * world_size
        dist.all_gather_object(allp, per)
        dist.all_gather_object(allpar, mine)
        bad = [n for n in fs.names if any(p[n] != allp[0][n] for p in allp)]
        worst = max(float((t - allpar[0]).abs().max()) for t in allpar)
        raise RuntimeError(f"epoch {epoch}: replicas diverged across ranks ({allg}); differing tensors "
                           f"{bad}, max |diff| {worst:.3e}")
    if rank == 0:
        tail = "" if getattr(opt, "ema", None) is None else f", weight EMA {ema_digest(opt.ema)[:12]}"
        print(f"Rank 0: replicas bitwise identical after epoch {epoch} ({d[:12]}{tail})", flush=True)


def _fault_step(fault, epoch, rank):
    if not fault:
        return None
    fe, fs_, fr = (list(fault) + [-1])[:3]
    return int(fs_) if int(fe) == epoch and int(fr) in (-1, rank) else None


def _inject_fault(rank, epoch, step):
    """Simulated hard failure: the rank dies without cleanup, as a crash
    would; the launcher tears the job down and a re-run auto-resumes from the last
    checkpoint."""
    print(f"Rank {rank}: injected fault at epoch {epoch} step {step}", flush=True)
    os._exit(17)


def _verify_and_broadcast(fs, model, world_size):
    """DDP construction semantics for the engine path: shape check + rank-0 broadcast."""
    if world_size == 1:
        return
    meta = [(n, fs.shapes[n]) for n in fs.names]
    allm = [None] * world_size
    dist.all_gather_object(allm, meta)
    if any(m != allm[0] for m in allm):
        raise RuntimeError(f"parameter shapes differ across ranks: {allm}")
    with torch.no_grad():
        dist.broadcast(fs.params, src=0)  # one flat collective (SimpleCNN has no buffers)
        fs.params_written()
        bs = buffer_space(model)
        if bs is not None:
            for t in bs.flat_list():  # one flat collective per dtype
                dist.broadcast(t, src=0)


_SYNC_EACH_STEP = os.environ.get("DDP_AMD_SYNC_EACH_STEP") == "1"
_VERIFY_EACH_STEP = os.environ.get("DDP_AMD_VERIFY_EACH_STEP") == "1"


def _verify_step(model, opt, step):
    """Diagnostic (DDP_AMD_VERIFY_EACH_STEP=1): compare the reduced gradients and the
    parameters across ranks after every step; raise at the first difference."""
    import hashlib

    fs = model.fs if hasattr(model, "fs") else flat_space(model)
    torch.cuda.synchronize()
    h = lambda t: hashlib.sha1(t.detach().cpu().numpy().tobytes()).hexdigest()[:10]  # noqa: E731
    mine = {"grads": {n: h(fs.view(fs.grads, n)) for n in fs.names}, "params": h(fs.params)}
    allm = [None] * dist.get_world_size()
    dist.all_gather_object(allm, mine)
    bad = [n for n in fs.names if any(m["grads"][n] != allm[0]["grads"][n] for m in allm)]
    if bad or any(m["params"] != allm[0]["params"] for m in allm):
        raise RuntimeError(f"step {step}: replicas differ - reduced gradients {bad}, params "
                           f"{[m['params'] for m in allm]}")


def _run_module_epoch(model, loader, loss_fn, opt, device, log, log_every, max_steps,
                      grad_accum=1, global_loss=False, graph=False):
    """The reference's loop (train_ddp.py:195-202).  With ``grad_accum`` > 1 the
    optimizer steps every ``grad_accum`` batches; the first ``grad_accum - 1`` backward
    passes run under ``no_sync`` (no all-reduce) and the loss is scaled so the update
    equals one large-batch step.  A ragged tail still flushes with a synchronised
    backward.  ``graph``: full-batch steps replay one captured hipGraph (GraphedStep;
    its capture warm-up steps are real steps on the first batch); a ragged last batch
    runs eagerly."""
    if graph:
        if grad_accum != 1 or global_loss:
            raise ValueError("--graph_module runs one micro-batch per step without loss all-reduce")
        return _run_graphed_epoch(model, loader, loss_fn, opt, log, log_every, max_steps)
    n = 0
    nb = len(loader) if hasattr(loader, "__len__") else None
    if max_steps is not None:
        nb = max_steps if nb is None else min(nb, max_steps)
    opt.zero_grad()
    for batch_idx, batch in enumerate(loader):
        images, labels = batch if isinstance(batch, (tuple, list)) else tuple(batch)
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)  # a PairTarget moves field by field
        if grad_accum == 1:
            opt.zero_grad()
        last = nb is not None and batch_idx + 1 >= nb
        boundary = grad_accum == 1 or (batch_idx + 1) % grad_accum == 0 or last
        output = model(images)
        loss = loss_fn(output, labels)
        scaled = loss / grad_accum if grad_accum > 1 else loss
        if boundary or not hasattr(model, "no_sync"):
            scaled.backward()
        else:
            with model.no_sync():
                scaled.backward()
        if boundary:
            opt.step()
            if grad_accum > 1:
                opt.zero_grad()
        if _SYNC_EACH_STEP:  # diagnostic: device-synchronise every step
            torch.cuda.synchronize()
        if _VERIFY_EACH_STEP and dist.is_initialized() and dist.get_world_size() > 1:
            _verify_step(model, opt, batch_idx)
        if batch_idx % log_every == 0:
            lv = loss.detach()
            if global_loss and dist.is_initialized() and dist.get_world_size() > 1:
                lv = lv.clone()
                dist.all_reduce(lv)
                lv = lv / dist.get_world_size()
            log(batch_idx, lv.item())
        n += 1
        if max_steps is not None and n >= max_steps:
            break
    return n


class _GraphCache(dict):
    """{input shape: GraphedStep} of one model (a dict subclass so it is weak-referenceable)."""


def _graph_cache(model) -> dict:
    """The model's captured training-step graphs, keyed by input shape.  Kept ON the model
    object (not in a module global keyed by ``id(model)``): it dies with the model, and a
    recycled id can never replay another model's graph."""
    cache = getattr(model, "_ddp_amd_step_graphs", None)
    if cache is None:
        cache = _GraphCache()
        object.__setattr__(model, "_ddp_amd_step_graphs", cache)
    return cache


def _run_graphed_epoch(model, loader, loss_fn, opt, log, log_every, max_steps):
    from .graph_step import GraphedStep

    from ..data.mix import PairTarget

    def step(x, *target):  # (y,) or a PairTarget's (y_a, y_b, w): every field a static input
        opt.zero_grad()
        loss = loss_fn(model(x), PairTarget(*target) if len(target) == 3 else target[0])
        loss.backward()
        opt.step()
        return loss

    graphs = _graph_cache(model)
    full = getattr(loader, "batch_size", None)  # the full batch: only that shape is captured
    n = 0
    for batch_idx, (images, labels) in enumerate(loader):
        target = tuple(labels) if isinstance(labels, PairTarget) else (labels,)
        key = tuple(images.shape) + (len(target),)
        if key not in graphs:
            if full is not None and images.shape[0] != full:
                loss = step(images, *target)  # ragged tail: eager, no new capture
            else:
                graphs[key] = GraphedStep(step, (images, *target), warmup=1)  # = this batch's step
                loss = graphs[key].warmup_out
        else:
            loss = graphs[key](images, *target)
        if batch_idx % log_every == 0:
            log(batch_idx, loss.item())
        n += 1
        if max_steps is not None and n >= max_steps:
            break
    return n


def samples_processed(nsteps: int, batch: int, samples_per_rank: int) -> int:
    """Images a rank actually trained on in ``nsteps`` steps of an epoch of
    ``samples_per_rank`` (full batches, then the ragged tail; ``--max_steps`` /
    ``--fault_at`` truncate the epoch)."""
    return min(nsteps * batch, samples_per_rank)


def _record_metrics(opts, rank, ws, epoch, nsteps, batch, dt, samples, ev=None, clip=None, lr=None, trust=None,
                    ev_ema=None, ema_updates=None):
    """``samples``: images this rank processed in the epoch (:func:`samples_processed`);
    ``ev``: the epoch's evaluation totals, when it ran (eval_loss / eval_accuracy keys);
    ``clip``: FusedSGD.grad_clip_stats() with --clip_grad_norm (grad_norm: the last step's
    norm; clipped_steps: steps clipped so far in this run); ``trust``: FusedLARS.trust_stats()
    (trust_ratio_min / trust_ratio_max over the adapted tensors, the epoch's last step);
    ``ev_ema``: the evaluation totals of the averaged weights with --eval_ema (eval_ema_* keys);
    ``ema_updates``: WeightEMA.num_updates() with --ema_decay."""
    if not opts.metrics_json or rank != 0:
        return
    import json

    rec = {"epoch": epoch, "world_size": ws, "steps": nsteps, "batch_size": batch,
           "samples_per_rank": samples, "seconds": dt,
           "images_per_sec_aggregate": samples * ws / dt if dt > 0 else None}
    if ev is not None:
        rec["eval_loss"], rec["eval_accuracy"] = ev.mean_loss, ev.accuracy
        if ev.correct5 is not None:
            rec["eval_top5"] = ev.top5
    if ev_ema is not None:
        rec["eval_ema_loss"], rec["eval_ema_accuracy"] = ev_ema.mean_loss, ev_ema.accuracy
        if ev_ema.correct5 is not None:
            rec["eval_ema_top5"] = ev_ema.top5
    if opts.label_smoothing:
        rec["label_smoothing"] = opts.label_smoothing
    if uses_augment(opts):
        rec["augment"] = augment_tag(opts)
    if uses_mix(opts):
        rec["mix"] = build_mix(opts).describe()
    if ema_updates is not None:
        rec["ema_updates"] = ema_updates
    if clip is not None:
        rec["grad_norm"], rec["clipped_steps"] = clip["total_norm"], clip["clipped"]
    if lr is not None:
        rec["lr"] = lr  # with a schedule: FusedSGD.current_lr() at the end of the epoch, the next step's rate
    if trust:
        ratios = [t["ratio"] for t in trust.values() if t["adapted"]]
        if ratios:
            rec["trust_ratio_min"], rec["trust_ratio_max"] = min(ratios), max(ratios)
    with open(opts.metrics_json, "a") as f:
        f.write(json.dumps(rec) + "\n")
