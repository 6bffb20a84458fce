"""Time the mixing gather against the plain and the augmenting gather, the PAIR cross-entropy
against the plain one, and the graphed ResNet-18 step fed through the loader with mixup / cutmix
off and on (profiles/mix/README.md).

    python scripts/mix_bench.py [--out profiles/mix/mix_bench.jsonl] [--skip_step]

Kernels: B = 32, 224 x 224, 2048 resident images (the loss: B = 32, C = 1000), the variants
alternating inside one process, device events around ``--iters`` launches per round.  Bytes are
the algorithm's: 8 written per output pixel, 3 read per source pixel a run needs (mixup: both
images; cutmix: the image each pixel comes from); the share of HBM bandwidth is against 8 TB/s.
Needs a GPU: there is no fall-back.
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


def timed(variants, iters, rounds):
    import torch

    for f in variants.values():  # warm-up: code objects loaded
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / iters)  # us per launch
    return {k: sorted(t) for k, t in times.items()}


def kernels(args):
    import torch

    from ddp_amd import native
    from ddp_amd.data import IMAGENET_MEAN, IMAGENET_STD, Augment, affine_table, mix_table, synthetic_imagenet

    C = native.require()
    dev = torch.device("cuda", 0)
    n, S, B = args.images, args.size, args.batch
    imgs = synthetic_imagenet(n, S, 1000)[0].to(dev)
    idx = torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(0)).to(dev)
    out = torch.empty(B, S, S, 4, dtype=torch.bfloat16, device=dev)
    aff = affine_table(IMAGENET_MEAN, IMAGENET_STD)
    rrc = Augment(rrc=True, flip=True).plan(0, n, S, S).rows.to(dev)
    partner = (torch.arange(B) - 1) % B
    q = S // 4  # a centred box of a quarter of the area
    tables = {"mixup": mix_table(partner, torch.zeros(B, 4), torch.full((B,), 0.3)).to(dev),
              "cutmix": mix_table(partner, torch.tensor([q, q, 3 * q, 3 * q]).expand(B, 4), torch.ones(B)).to(dev),
              "unmixed": mix_table(partner, torch.zeros(B, 4), torch.ones(B)).to(dev)}
    variants = {"plain": lambda: C.image_gather_nhwc4(imgs, idx, out),
                "rrc+flip+norm": lambda: C.image_gather_aug_nhwc4(imgs, idx, rrc, aff, out, True)}
    for k, t in tables.items():
        variants[f"rrc+flip+norm+{k}"] = lambda t=t: C.image_gather_mix_nhwc4(imgs, idx, rrc, aff, t, out, True)
    reads = {"plain": 3, "rrc+flip+norm": 3, "rrc+flip+norm+mixup": 6, "rrc+flip+norm+cutmix": 3,
             "rrc+flip+norm+unmixed": 3}
    recs = []
    for k, t in timed(variants, args.iters, args.rounds).items():
        med, nbytes = t[len(t) // 2], B * S * S * (reads[k] + 8)
        recs.append({"bench": "gather_kernel", "variant": k, "batch": B, "size": S, "images": n, "us_median": med,
                     "us_min": t[0], "us_max": t[-1], "bytes": nbytes, "tb_per_s": nbytes / med * 1e-6,
                     "hbm_share": nbytes / (med * 1e-6) / HBM_PEAK})
    # the loss: xent_wave_rows_kernel plain against PAIR, with label smoothing 0.1
    Cn = 1000
    g = torch.Generator().manual_seed(1)
    lg = torch.randn(B, Cn, generator=g).to(dev)
    ya, yb = (torch.randint(0, Cn, (B,), generator=g).to(dev) for _ in range(2))
    w = torch.tensor([[0.3, 0.7]]).expand(B, 2).contiguous().to(dev)
    dl, loss = torch.empty_like(lg), torch.empty(1, device=dev)
    xv = {"xent": lambda: C.xent(lg, 1, None, ya, None, dl, loss, None, 1.0 / B, 0.0, label_smoothing=0.1),
          "xent_pair": lambda: C.xent(lg, 1, None, ya, None, dl, loss, None, 1.0 / B, 0.0, label_smoothing=0.1,
                                      labels_b=yb, pair_w=w)}
    for k, t in timed(xv, args.iters, args.rounds).items():
        recs.append({"bench": "xent_kernel", "variant": k, "batch": B, "classes": Cn, "us_median": t[len(t) // 2],
                     "us_min": t[0], "us_max": t[-1]})
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
            "native_so": os.environ.get("DDP_AMD_NATIVE_SO", "(in-tree)"),
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
    p.add_argument("--skip_kernels", action="store_true")
    args = p.parse_args()
    recs = [] if args.skip_kernels else kernels(args)
    if not args.skip_step:
        base = ["--aug_rrc", "--aug_flip", "--normalize", "--label_smoothing", "0.1"]
        mixed = base + ["--mixup_alpha", "0.2", "--cutmix_alpha", "1.0"]
        for flags in (base, mixed, base, mixed):
            recs.append(step(flags, args))
    for r in recs:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in recs)


if __name__ == "__main__":
    main()
