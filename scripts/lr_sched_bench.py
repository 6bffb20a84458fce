"""Cost of a learning-rate schedule (FusedSGD(lr_schedule=), the DLR build of sgd_kernel),
measured in ONE call (same process, same clocks, alternating pairs):

* the bare ``sgd_kernel`` at ResNet-18's flat parameter count as the ResNet step runs it
  (momentum 0.9 + the bf16 shadow), by-value rate against the device-resident table, each also
  with the clip coefficient - in-graph time per launch as scripts/kbench.py measures it;
* the ResNet-18 graphed training step (batch 32, 224 x 224) with the schedule off and on.

    python scripts/lr_sched_bench.py [--reps 20] [--iters 10] [--rounds 5] [--steps 20] [--json out.jsonl]
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
from ddp_amd.ops.lr_schedule import LRSchedule  # noqa: E402
from kbench import timed  # noqa: E402  (scripts/ is sys.path[0] when run as a script)


def kernel_times(C, n, a, emit):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    gr = torch.randn(n, device=dev, generator=g) * 1e-3
    mb = torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    coef = torch.ones(1, device=dev)
    table = torch.full((1000,), 1e-6, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    shadow = [(0, n, sh, 1, 0, 0, 0)]

    def sgd(gscale, sched):
        return lambda: C.sgd(p, gr, mb, 1e-6, 0.9, 0.0, 0.0, False, False, False, True, shadow, gscale, sched)

    variants = {
        "sgd by value": sgd(None, None),
        "sgd DLR": sgd(None, (table, state)),
        "sgd CLIP by value": sgd(coef, None),
        "sgd CLIP DLR": sgd(coef, (table, state)),
        "noop": lambda: C.noop(2048),
    }
    us = {k: [] for k in variants}
    for _ in range(a.rounds):  # alternate: every variant once per round
        for k, fn in variants.items():
            us[k].append(timed(fn, a.reps, a.iters))
    s = state.cpu()
    for k, v in us.items():
        emit({"bench": "kernel", "name": k, "n": n, "us": statistics.median(v), "us_rounds": v})
    emit({"bench": "kernel", "name": "DLR state", "t": int(s[0]), "ticket": int(s[1])})
    return {k: statistics.median(v) for k, v in us.items()}


def step_times(a, emit):
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    dev = torch.device("cuda", 0)
    B = a.batch
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)

    def make(schedule):
        torch.manual_seed(0)
        model = resnet18(num_classes=1000).to(dev)
        opt = FusedSGD(model, lr=0.01, momentum=0.9, lr_schedule=schedule)
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return GraphedStep(step, (x, y), warmup=2), opt

    total = 2 + a.rounds * (a.steps + 1)
    runs = {"schedule off": make(None),
            "cosine + warm-up": make(LRSchedule(0.01, total, "cosine", warmup_steps=5, lr_min=1e-5))}
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
               "img_per_s_rounds": v, "ms_per_step": 1e3 * B / statistics.median(v)}
        if runs[k][1].lr_schedule is not None:
            rec["schedule_step"], rec["total_steps"] = runs[k][1].schedule_step(), total
        emit(rec)
    return runs["schedule off"][1].flat.numel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
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
    kernel_times(C, a.n or n, a, emit)


if __name__ == "__main__":
    main()
