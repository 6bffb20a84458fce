"""Cost of --clip_grad_norm, measured in ONE call (same process, same clocks, alternating rounds):

* ``grad_sqnorm`` (csrc/kernels/grad_norm.hip) against the existing ``sgd_kernel`` at
  ResNet-18's flat parameter count - in-graph time per launch as scripts/kbench.py measures
  it, with the norm kernel's achieved read bandwidth.  The SGD pass is timed in its lightest
  form (no momentum, no shadow: 12 bytes per element against the norm's 4) and as the ResNet
  step runs it (momentum 0.9 + the bf16 shadow), plus the CLIP build of the latter;
* the ResNet-18 graphed training step (batch 32, 224 x 224) with and without clipping.

    python scripts/clip_bench.py [--reps 20] [--iters 10] [--rounds 3] [--steps 20] [--json out.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ddp_amd import native  # noqa: E402
from kbench import timed  # noqa: E402  (scripts/ is sys.path[0] when run as a script)


def kernel_times(C, n, a, emit):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    gr = torch.randn(n, device=dev, generator=g) * 1e-3
    mb = torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    partials = torch.zeros(C.GRAD_NORM_MAX_BLOCKS, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.zeros(4, device=dev)
    shadow = [(0, n, sh, 1, 0, 0, 0)]
    variants = {
        "grad_sqnorm": lambda: C.grad_sqnorm(gr, 1.0, partials, ticket, stats),
        "sgd plain": lambda: C.sgd(p, gr, None, 1e-6, 0.0, 0.0, 0.0, False, False, False, True, []),
        "sgd momentum+bf16 shadow": lambda: C.sgd(p, gr, mb, 1e-6, 0.9, 0.0, 0.0, False, False, False, True, shadow),
        "sgd momentum+bf16 shadow CLIP": lambda: C.sgd(p, gr, mb, 1e-6, 0.9, 0.0, 0.0, False, False, False, True,
                                                       shadow, stats[1:2]),
        "noop": lambda: C.noop(C.grad_norm_blocks(n)),
    }
    us = {k: [] for k in variants}
    for _ in range(a.rounds):  # alternate: every variant once per round
        for k, fn in variants.items():
            us[k].append(timed(fn, a.reps, a.iters))
    for k, v in us.items():
        rec = {"bench": "kernel", "name": k, "n": n, "us": statistics.median(v), "us_rounds": v}
        if k == "grad_sqnorm":
            rec["GBps"] = 4.0 * n / (rec["us"] * 1e-6) / 1e9
        emit(rec)
    return {k: statistics.median(v) for k, v in us.items()}


def step_times(a, emit):
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    dev = torch.device("cuda", 0)
    B = a.batch
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)

    def make(clip):
        torch.manual_seed(0)
        model = resnet18(num_classes=1000).to(dev)
        opt = FusedSGD(model, lr=0.01, momentum=0.9, max_grad_norm=clip)
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return GraphedStep(step, (x, y), warmup=2), opt

    runs = {"unclipped": make(None), "clip 1.0": make(1.0)}
    ips = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (gs, _) in runs.items():
            gs(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gs(x, y)
            torch.cuda.synchronize()
            ips[k].append(a.steps * B / (time.perf_counter() - t0))
    for k, v in ips.items():
        rec = {"bench": "resnet18 graphed step", "name": k, "batch": B, "img_per_s": statistics.median(v),
               "img_per_s_rounds": v}
        if runs[k][1].max_grad_norm is not None:
            rec["clip_stats"] = runs[k][1].grad_clip_stats()
        emit(rec)
    return runs["unclipped"][1].flat.numel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n", type=int, default=0, help="flat size (0: ResNet-18's, from the model)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    C = native.require()
    out = open(a.json, "a") if a.json else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n = step_times(a, emit)
    t = kernel_times(C, a.n or n, a, emit)
    emit({"bench": "condition", "grad_sqnorm_us": t["grad_sqnorm"], "sgd_plain_us": t["sgd plain"],
          "norm_not_slower_than_sgd": t["grad_sqnorm"] <= t["sgd plain"]})


if __name__ == "__main__":
    main()
