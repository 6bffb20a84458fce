"""Time the augmenting gather against the plain gather, and the graphed ResNet-18 step fed
through the loader with the augmentation off and on (profiles/augment/README.md).

    python scripts/aug_bench.py [--out profiles/augment/aug_bench.jsonl] [--skip_step]

Kernels: B = 32, 224 x 224, 2048 resident images, the three variants alternating inside one
process, device events around ``--iters`` launches per round, fresh random indices and a fresh
plan per variant.  Bytes are the algorithm's (3 read + 8 written per output pixel); the share
of HBM bandwidth is against 8 TB/s.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK = 8.0e12


def kernels(args):
    import torch

    from ddp_amd import native
    from ddp_amd.data import IMAGENET_MEAN, IMAGENET_STD, Augment, affine_table, synthetic_imagenet

    C = native.require()
    dev = torch.device("cuda", 0)
    n, S, B = args.images, args.size, args.batch
    imgs = synthetic_imagenet(n, S, 1000)[0].to(dev)
    idx = torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(0)).to(dev)
    out = torch.empty(B, S, S, 4, dtype=torch.bfloat16, device=dev)
    aff = affine_table(IMAGENET_MEAN, IMAGENET_STD)
    crop = Augment(crop_pad=4, flip=True).plan(0, n, S, S).rows.to(dev)
    rrc = Augment(rrc=True, flip=True).plan(0, n, S, S).rows.to(dev)
    variants = {"plain": lambda: C.image_gather_nhwc4(imgs, idx, out),
                "crop+flip+norm": lambda: C.image_gather_aug_nhwc4(imgs, idx, crop, aff, out, False),
                "rrc+flip+norm": lambda: C.image_gather_aug_nhwc4(imgs, idx, rrc, aff, out, True)}
    for f in variants.values():  # warm-up: code objects loaded
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / args.iters)  # us per launch
    nbytes = B * S * S * (3 + 8)
    recs = []
    for k, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        recs.append({"bench": "gather_kernel", "variant": k, "batch": B, "size": S, "images": n, "us_median": med,
                     "us_min": t[0], "us_max": t[-1], "bytes": nbytes, "tb_per_s": nbytes / med * 1e-6,
                     "hbm_share": nbytes / (med * 1e-6) / HBM_PEAK})
    return recs


def step(flags, args):
    """img/s of the last epoch of a graphed ResNet-18 run through the CLI (batch 32, 2048 images)."""
    with tempfile.TemporaryDirectory() as d:
        mj = os.path.join(d, "m.jsonl")
        cmd = [sys.executable, os.path.join(REPO, "train_ddp.py"), "--model", "resnet18", "--world_size", "1",
               "--epochs", str(args.epochs), "--batch_size", str(args.batch), "--graph_module", "--no_save",
               "--checkpoint_dir", os.path.join(d, "ck"), "--metrics_json", mj, *flags]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=args.step_timeout)
        recs = [json.loads(line) for line in open(mj)]
    return {"bench": "resnet18_graphed_step", "flags": " ".join(flags) or "(none)", "batch": args.batch,
            "img_per_s_last_epoch": recs[-1]["images_per_sec_aggregate"],
            "img_per_s_epochs": [r["images_per_sec_aggregate"] for r in recs]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--images", type=int, default=2048)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--step_timeout", type=float, default=240.0)
    p.add_argument("--skip_step", action="store_true")
    args = p.parse_args()
    recs = kernels(args)
    if not args.skip_step:
        for flags in ([], ["--aug_rrc", "--aug_flip", "--normalize"], [], ["--aug_rrc", "--aug_flip", "--normalize"]):
            recs.append(step(flags, args))
    for r in recs:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in recs)


if __name__ == "__main__":
    main()
