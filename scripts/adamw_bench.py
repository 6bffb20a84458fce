"""Cost of AdamW (FusedAdamW, adamw_kernel) against SGD, measured in ONE call (same process,
same clocks, alternating pairs):

* the bare ``adamw_kernel`` at ResNet-18's flat parameter count with the bf16 shadow, against
  ``sgd_kernel`` with momentum 0.9 by value and against its DLR build ``sgd_kernel<false, true>``
  (the same ticket protocol) - in-graph time per launch as scripts/kbench.py measures it;
* the ResNet-18 graphed training step (batch 32, 224 x 224), ``FusedSGD(momentum=0.9)`` against
  ``FusedAdamW``.

    python scripts/adamw_bench.py [--reps 20] [--iters 10] [--rounds 5] [--steps 20] [--json out.jsonl]
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
from ddp_amd.ops.adamw import coef_table  # noqa: E402
from kbench import timed  # noqa: E402  (scripts/ is sys.path[0] when run as a script)


def kernel_times(C, n, a, emit):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    gr = torch.randn(n, device=dev, generator=g) * 1e-3
    mb = torch.zeros(n, device=dev)
    vb = torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    coef = torch.ones(1, device=dev)
    table = torch.full((1000,), 1e-6, device=dev)
    ctab = coef_table(1e-6, (0.9, 0.999), 0.0).to(dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    astate = torch.zeros(4, dtype=torch.int32, device=dev)
    shadow = [(0, n, sh, 1, 0, 0, 0)]

    def sgd(gscale, sched):
        return lambda: C.sgd(p, gr, mb, 1e-6, 0.9, 0.0, 0.0, False, False, False, True, shadow, gscale, sched)

    def adamw(gscale):
        return lambda: C.adamw(p, gr, mb, vb, 0.9, 0.999, 1e-8, False, True, shadow, gscale, (ctab, astate))

    variants = {
        "sgd momentum by value": sgd(None, None),
        "sgd momentum DLR": sgd(None, (table, state)),
        "adamw": adamw(None),
        "adamw CLIP": adamw(coef),
        "noop": lambda: C.noop(2048),
    }
    us = {k: [] for k in variants}
    for _ in range(a.rounds):  # alternate: every variant once per round
        for k, fn in variants.items():
            us[k].append(timed(fn, a.reps, a.iters))
    for k, v in us.items():
        emit({"bench": "kernel", "name": k, "n": n, "us": statistics.median(v), "us_rounds": v})
    s = astate.cpu()
    emit({"bench": "kernel", "name": "adamw state", "t": int(s[0]), "ticket": int(s[1])})
    # bytes per element: sgd reads p, g, m and writes p, m (+ 2-byte shadow); adamw reads p, g, m, v
    # and writes p, m, v (+ shadow)
    emit({"bench": "kernel", "name": "bytes", "sgd_bytes_per_elem": 22, "adamw_bytes_per_elem": 30,
          "byte_ratio": 30 / 22})
    return {k: statistics.median(v) for k, v in us.items()}


def step_times(a, emit):
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedAdamW, FusedSGD

    dev = torch.device("cuda", 0)
    B = a.batch
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)

    def make(kind):
        torch.manual_seed(0)
        model = resnet18(num_classes=1000).to(dev)
        opt = FusedSGD(model, lr=0.01, momentum=0.9) if kind == "sgd" else FusedAdamW(model, lr=1e-3)
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return GraphedStep(step, (x, y), warmup=2), opt

    runs = {"sgd": make("sgd"), "adamw": make("adamw")}
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
        if k == "adamw":
            rec["adam_step"], rec["expected_steps"] = runs[k][1].schedule_step(), 2 + a.rounds * (a.steps + 1)
        emit(rec)
    return runs["sgd"][1].flat.numel


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
