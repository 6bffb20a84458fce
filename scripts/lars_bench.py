"""Cost of LARS (FusedLARS: seg_sqnorm_kernel + lars_kernel) against SGD, measured in ONE call
(same process, same clocks, alternating rounds):

* at ResNet-18's flat layout (its real segment table), ``seg_sqnorm_kernel`` and ``lars_kernel``
  with the bf16 shadow, beside ``sgd_kernel`` (momentum 0.9, by value) and ``grad_sqnorm_kernel``
  - in-graph time per launch as scripts/kbench.py measures it.  Expectation by bytes: the norm
  kernel reads w and g once (8 B per element) against g alone (4 B) for the clip norm; the update
  kernel moves sgd_kernel's 22 B per element plus one 2-byte chunk-map entry per 64 elements;
* the ResNet-18 graphed training step (batch 32, 224 x 224), ``FusedSGD(momentum=0.9)`` against
  ``FusedLARS(momentum=0.9)``.

    python scripts/lars_bench.py [--reps 20] [--iters 10] [--rounds 5] [--steps 20] [--json out.jsonl]
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


def kernel_times(C, lars_opt, a, emit):
    dev = "cuda"
    n = lars_opt.flat.numel
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    gr = torch.randn(n, device=dev, generator=g) * 1e-3
    mb = torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    shadow = [(0, n, sh, 1, 0, 0, 0)]
    plan, partials, ticket, sums, trust = lars_opt._workspace(C)
    cpart = torch.zeros(C.GRAD_NORM_MAX_BLOCKS, device=dev)
    cticket = torch.zeros(1, dtype=torch.int32, device=dev)
    cstats = torch.zeros(4, device=dev)
    variants = {
        "sgd momentum by value": lambda: C.sgd(p, gr, mb, 1e-6, 0.9, 0.0, 0.0, False, False, False, True, shadow, None, None),
        "lars": lambda: C.lars(p, gr, mb, 1e-6, 0.9, 0.0, False, False, False, True, shadow, plan, trust, None, None),
        "grad_sqnorm": lambda: C.grad_sqnorm(gr, 1.0, cpart, cticket, cstats),
        "seg_sqnorm": lambda: C.seg_sqnorm(p, gr, plan, partials, ticket, sums, trust, 1e-3, 1e-8, None),
        "noop": lambda: C.noop(2048),
    }
    us = {k: [] for k in variants}
    for _ in range(a.rounds):  # alternate: every variant once per round
        for k, fn in variants.items():
            us[k].append(timed(fn, a.reps, a.iters))
    for k, v in us.items():
        emit({"bench": "kernel", "name": k, "n": n, "us": statistics.median(v), "us_rounds": v})
    n_seg, n_items = plan[0].shape[0], plan[1].shape[0]
    emit({"bench": "kernel", "name": "table", "tensors": n_seg, "work_items": n_items, "chunks": plan[2].numel(),
          "seg_sqnorm_blocks": C.seg_sqnorm_blocks(n_items)})
    emit({"bench": "kernel", "name": "bytes", "sgd_bytes_per_elem": 22, "lars_bytes_per_elem": 22 + 2 / 64,
          "grad_sqnorm_bytes_per_elem": 4, "seg_sqnorm_bytes_per_elem": 8})


def step_times(a, emit):
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedLARS, FusedSGD

    dev = torch.device("cuda", 0)
    B = a.batch
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)

    def make(kind):
        torch.manual_seed(0)
        model = resnet18(num_classes=1000).to(dev)
        opt = (FusedSGD(model, lr=0.01, momentum=0.9) if kind == "sgd" else
               FusedLARS(model, lr=0.01, momentum=0.9, weight_decay=1e-4))
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return GraphedStep(step, (x, y), warmup=2), opt

    runs = {"sgd": make("sgd"), "lars": make("lars")}
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
        if k == "lars":
            ratios = [t["ratio"] for t in runs[k][1].trust_stats().values() if t["adapted"]]
            rec["trust_ratio_min"], rec["trust_ratio_max"] = min(ratios), max(ratios)
        emit(rec)
    return runs["lars"][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
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

    opt = step_times(a, emit)
    kernel_times(C, opt, a, emit)


if __name__ == "__main__":
    main()
