"""DDP trainer CLI - drop-in for the reference's ``train_ddp.py``.

    python train_ddp.py [--epochs 10] [--batch_size 32] [--world_size N]
    torchrun --nproc_per_node=N train_ddp.py --epochs 3 --batch_size 64

Same flags and defaults as the reference (train_ddp.py:215-219: ``--epochs``
10, per-rank ``--batch_size`` 32) plus the README's documented ``--world_size``
(reference bug B1) and MI355X options.  Under torchrun the ranks come from the
environment (no nested spawn, bug B3); otherwise ``--world_size`` processes are
spawned (default: all visible GPUs, or 2 on a CPU host).  Checkpoints go to
``./checkpoints/epoch_{N}.pt`` and a re-run resumes from the newest one.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ddp_amd.engine.trainer import TrainOptions, ddp_train, validate_options  # noqa: E402
from ddp_amd.parallel.launcher import launch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="DDP Training Script (MI355X-native)")
    p.add_argument("--epochs", type=int, default=10, help="Number of training epochs")
    p.add_argument("--batch_size", type=int, default=32, help="Batch size for training (per rank)")
    p.add_argument("--world_size", type=int, default=None,
                   help="processes to spawn when not under torchrun (default: #GPUs, or 2 on CPU)")
    p.add_argument("--backend", choices=["rccl", "nccl", "gloo"], default=None,
                   help="collective backend (default: rccl on GPU, gloo on CPU)")
    p.add_argument("--device", choices=["auto", "gpu", "cpu"], default="auto",
                   help="gpu: fail unless a HIP device is usable; cpu: gloo plumbing run; auto: the GPU "
                        "when usable, CPU only on a host without one (never a silent fallback on a GPU host)")
    p.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16",
                   help="GPU compute precision: bf16 MFMA operands (fp32 masters/grads/optimizer) or "
                        "exact fp32 MFMA (the reference's fp32 nn.Conv2d/nn.Linear precision)")
    p.add_argument("--engine", choices=["fused", "module"], default="fused",
                   help="GPU step: fused native engine (hipGraph) or module path (autograd)")
    p.add_argument("--data", choices=["auto", "mnist", "synthetic"], default="auto",
                   help="MNIST IDX files under --data_root if present, else synthetic MNIST-shaped")
    p.add_argument("--data_root", default="./data")
    p.add_argument("--checkpoint_dir", default="./checkpoints")
    p.add_argument("--no_save", action="store_true", help="do not write checkpoints")
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--momentum", type=float, default=0.0)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--optimizer", choices=["sgd", "adamw", "lars"], default="sgd",
                   help="sgd: torch.optim.SGD semantics (--momentum); adamw: torch.optim.AdamW semantics "
                        "(--beta1 / --beta2 / --adam_eps, decoupled --weight_decay), one fused kernel whose "
                        "bias correction follows a device step counter, so --graph_module replays are exact "
                        "(module/CPU path); lars: SGD with --momentum whose per-tensor decayed gradient is scaled "
                        "by a trust ratio computed on the device (--trust_coef / --lars_eps / --lars_exclude; "
                        "module/CPU path)")
    p.add_argument("--beta1", type=float, default=0.9, help="adamw: first-moment decay")
    p.add_argument("--beta2", type=float, default=0.999, help="adamw: second-moment decay")
    p.add_argument("--adam_eps", type=float, default=1e-8, help="adamw: the denominator's epsilon")
    p.add_argument("--trust_coef", type=float, default=1e-3, help="lars: the trust ratio's coefficient")
    p.add_argument("--lars_eps", type=float, default=1e-8, help="lars: the trust ratio denominator's epsilon")
    p.add_argument("--lars_exclude", choices=["1d", "none"], default="1d",
                   help="lars: 1d = parameters with ndim <= 1 (BatchNorm scales, biases) get ratio 1 and no "
                        "weight decay; none = every tensor is adapted and decayed")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log_every", type=int, default=100)
    p.add_argument("--graph_steps", type=int, default=100, help="steps per captured hipGraph")
    p.add_argument("--bucket_cap_mb", type=float, default=25.0)
    p.add_argument("--num_workers", type=int, default=2, help="CPU DataLoader workers")
    p.add_argument("--max_steps", type=int, default=None, help="cap steps per epoch (module/CPU path)")
    p.add_argument("--metrics_json", default=None, help="append per-epoch img/s records (rank 0)")
    p.add_argument("--fuse_level", type=int, default=None, choices=[0, 1, 3],
                   help="fused engine: 0 = a1 materialised, separate conv1/xent/dgrad/wgrad/SGD kernels; "
                        "1 = 3 kernels/step; 3 = dZ2 in the forward, fc weight gradient inside the conv "
                        "backward: 2 kernels/step (default)")
    p.add_argument("--comm", choices=["auto", "tune", "xgmi", "xgmi1", "xgmi2", "rccl"], default="auto",
                   help="bucket all-reduce data plane at world size > 1. Fused engine: auto = the direct xGMI "
                        "kernels (one-shot for the small bucket; RCCL if their self-test fails) - deterministic, "
                        "so resumes reduce in the same order; tune = fastest of xgmi2 / xgmi1 / RCCL on the "
                        "node. Module path (--engine module, resnet18): rccl, or xgmi for any xgmi* / tune; "
                        "auto = RCCL under the rccl backend, xGMI under gloo")
    p.add_argument("--grad_accum", type=int, default=1,
                   help="micro-batches per optimizer step (module/CPU path; DDP no_sync)")
    p.add_argument("--clip_grad_norm", type=float, default=0.0, metavar="X",
                   help="clip the global gradient L2 norm to X inside the optimizer step, as "
                        "torch.nn.utils.clip_grad_norm_ (module/CPU path; 0 = off)")
    p.add_argument("--label_smoothing", type=float, default=0.0, metavar="E",
                   help="train against the target (1 - E) * onehot + E / C over all C classes, as "
                        "torch.nn.CrossEntropyLoss(label_smoothing=E), inside the fused cross-entropy kernels "
                        "(module/CPU path; 0 = off; evaluation losses stay the plain cross-entropy)")
    p.add_argument("--lr_schedule", choices=["none", "cosine", "linear", "step"], default="none",
                   help="learning-rate decay per optimizer step over --epochs (after --warmup_steps): cosine or "
                        "linear down to --lr_min, or times --lr_gamma every --lr_step_epochs epochs; read on the "
                        "device, so --graph_module replays follow it (module/CPU path)")
    p.add_argument("--warmup_steps", type=int, default=0, metavar="N",
                   help="linear warm-up from 0.01 x --lr to --lr over the first N optimizer steps (module/CPU path)")
    p.add_argument("--lr_min", type=float, default=0.0, metavar="X", help="cosine / linear: the final rate")
    p.add_argument("--lr_step_epochs", type=int, default=0, metavar="N", help="step: epochs between decays")
    p.add_argument("--lr_gamma", type=float, default=0.1, metavar="G", help="step: decay factor")
    p.add_argument("--global_loss", action="store_true",
                   help="log the all-reduced mean loss instead of rank 0's local loss (module/CPU path)")
    p.add_argument("--pg_timeout_min", type=float, default=30.0,
                   help="process-group timeout in minutes (reference default 30)")
    p.add_argument("--model", choices=["simplecnn", "resnet18"], default="simplecnn",
                   help="resnet18 = BASELINE config 5 on synthetic ImageNet-shaped data (module path)")
    p.add_argument("--image_size", type=int, default=224, help="resnet18: synthetic image side")
    p.add_argument("--num_classes", type=int, default=1000, help="resnet18: classes")
    p.add_argument("--dataset_size", type=int, default=2048, help="resnet18: synthetic images")
    p.add_argument("--graph_module", action="store_true",
                   help="module path on GPU: replay each training step as one captured hipGraph")
    p.add_argument("--fault_at", default=None, metavar="EPOCH:STEP[:RANK]",
                   help="simulate a crash (os._exit) at that step; re-run to auto-resume")
    p.add_argument("--stall_at", default=None, metavar="EPOCH:RANK:SECONDS",
                   help="simulate a slow rank: it sleeps before that epoch's first step")
    p.add_argument("--force_allreduce", action="store_true",
                   help="rehearsal on one GPU: run the multi-GPU fused step chain at world size 1 (forked "
                        "fc branch, bucket all-reduces of the 8-rank plan on the --comm plane, chain check)")
    p.add_argument("--verify_replicas", action="store_true",
                   help="after every epoch check that all ranks' parameters and momentum are bitwise equal")
    p.add_argument("--eval_every", type=int, default=0,
                   help="evaluate the held-out test split (sharded over the ranks, exact counts) after every "
                        "Nth epoch; 0 = never (simplecnn; resnet18 with --eval_size)")
    p.add_argument("--eval_batch_size", type=int, default=1000, help="images per evaluation batch")
    p.add_argument("--eval_only", action="store_true",
                   help="resume from the newest checkpoint, evaluate the test split, exit")
    p.add_argument("--eval_size", type=int, default=0,
                   help="resnet18: build a synthetic held-out split of N images (at --image_size / --num_classes) "
                        "for --eval_every / --eval_only; 0 = none")
    p.add_argument("--ema_decay", type=float, default=0.0, metavar="D",
                   help="keep an exponential moving average of the weights, updated by one fused kernel at the "
                        "end of every optimizer step (inside --graph_module captures too) and saved in the "
                        "checkpoint's \"ema\" entry (module/CPU path; 0 = off)")
    p.add_argument("--ema_warmup", action="store_true",
                   help="ema: update k uses the decay min(D, (1 + k) / (10 + k)), read on the device, so "
                        "--graph_module replays follow it")
    p.add_argument("--eval_ema", action="store_true",
                   help="every --eval_every / --eval_only evaluation also evaluates the averaged weights "
                        "(an extra 'Eval EMA' line; BatchNorm statistics are the live ones)")
    p.add_argument("--normalize", action="store_true",
                   help="resnet18: normalise with the ImageNet mean / std inside every image gather, training "
                        "and evaluation alike (one fma per value in the gather kernel)")
    p.add_argument("--aug_crop_pad", type=int, default=0, metavar="P",
                   help="resnet18: random crop with P pixels of black padding, as torchvision's "
                        "RandomCrop(size, padding=P), inside the gather kernel (0 = off)")
    p.add_argument("--aug_rrc", action="store_true",
                   help="resnet18: random resized crop (area share --aug_scale_min..1, ratio 3/4..4/3, "
                        "bilinear) back to the stored size, inside the gather kernel; not with --aug_crop_pad")
    p.add_argument("--aug_scale_min", type=float, default=0.08, metavar="S",
                   help="aug_rrc: the smallest share of the image area a box takes, in (0, 1]")
    p.add_argument("--aug_flip", action="store_true",
                   help="resnet18: horizontal flip with p = 0.5 after the crop, inside the gather kernel")
    p.add_argument("--mixup_alpha", type=float, default=0.0, metavar="A",
                   help="resnet18: mixup - each batch is blended with itself rolled by one row, lam ~ Beta(A, A) "
                        "per batch, inside the gather kernel, and trains against the two labels' weighted "
                        "(label-smoothed) targets inside the cross-entropy kernels (0 = off)")
    p.add_argument("--cutmix_alpha", type=float, default=0.0, metavar="A",
                   help="resnet18: cutmix - a box of area share 1 - lam0, lam0 ~ Beta(A, A) per batch, shows "
                        "the rolled batch's pixels; the target weight follows the clipped area (0 = off)")
    p.add_argument("--mix_prob", type=float, default=1.0, metavar="P",
                   help="mixup / cutmix: the probability that a batch is mixed at all")
    p.add_argument("--mix_switch_prob", type=float, default=0.5, metavar="P",
                   help="with both alphas: the probability that a mixed batch is a cutmix batch")
    return p.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    opts = TrainOptions(lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay,
                        backend=a.backend, device=a.device, engine=a.engine, dtype=a.dtype, data=a.data, data_root=a.data_root,
                        checkpoint_dir=a.checkpoint_dir, save=not a.no_save, seed=a.seed,
                        log_every=a.log_every, graph_steps=a.graph_steps,
                        bucket_cap_mb=a.bucket_cap_mb, num_workers=a.num_workers,
                        max_steps=a.max_steps, metrics_json=a.metrics_json,
                        fuse_level=a.fuse_level, grad_accum=a.grad_accum,
                        global_loss=a.global_loss, pg_timeout_s=a.pg_timeout_min * 60.0,
                        comm=a.comm, model=a.model, image_size=a.image_size,
                        num_classes=a.num_classes, dataset_size=a.dataset_size,
                        graph_module=a.graph_module, verify_replicas=a.verify_replicas,
                        force_allreduce=a.force_allreduce, eval_every=a.eval_every,
                        eval_batch_size=a.eval_batch_size, eval_only=a.eval_only, eval_size=a.eval_size,
                        clip_grad_norm=a.clip_grad_norm, lr_schedule=a.lr_schedule,
                        warmup_steps=a.warmup_steps, lr_min=a.lr_min, lr_step_epochs=a.lr_step_epochs,
                        lr_gamma=a.lr_gamma, optimizer=a.optimizer, beta1=a.beta1, beta2=a.beta2,
                        adam_eps=a.adam_eps, trust_coef=a.trust_coef, lars_eps=a.lars_eps,
                        lars_exclude=a.lars_exclude, ema_decay=a.ema_decay, ema_warmup=a.ema_warmup,
                        eval_ema=a.eval_ema, label_smoothing=a.label_smoothing,
                        normalize=a.normalize, aug_crop_pad=a.aug_crop_pad, aug_rrc=a.aug_rrc,
                        aug_scale_min=a.aug_scale_min, aug_flip=a.aug_flip,
                        mixup_alpha=a.mixup_alpha, cutmix_alpha=a.cutmix_alpha, mix_prob=a.mix_prob,
                        mix_switch_prob=a.mix_switch_prob,
                        stall=tuple(float(v) for v in a.stall_at.split(":")) if a.stall_at else None,
                        fault=tuple(int(v) for v in a.fault_at.split(":")) if a.fault_at else None)
    validate_options(opts)
    launch(ddp_train, a.world_size, args=(a.epochs, a.batch_size, opts))


if __name__ == "__main__":
    main()
