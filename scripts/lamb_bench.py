"""Cost of LAMB (FusedLAMB: lamb_moments_kernel + lamb_apply_kernel) against AdamW and LARS,
measured in ONE call (same process, same clocks, alternating rounds):

* at ResNet-18's flat layout (its real segment table), the two LAMB kernels with the bf16 shadow,
  beside ``adamw_kernel`` and beside ``seg_sqnorm_kernel`` + ``lars_kernel`` - in-graph time per
  launch as scripts/kbench.py measures it.  Expectation by bytes per element (lamb.hip header):
  pass 1 reads 16 and writes 8, pass 2 reads 12 and writes 4 + 2: 42 against adamw_kernel's 30,
  plus one launch and the last-arrival tail of pass 1;
* the ResNet-18 graphed training step (batch 32, 224 x 224), ``FusedAdamW`` against ``FusedLAMB``.

    python scripts/lamb_bench.py [--reps 20] [--iters 10] [--rounds 5] [--steps 20] [--json out.jsonl]
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
from ddp_amd.ops.lamb import lamb_coef_table  # noqa: E402
from kbench import timed  # noqa: E402  (scripts/ is sys.path[0] when run as a script)


def kernel_times(C, lamb_opt, a, emit):
    dev = "cuda"
    n = lamb_opt.flat.numel
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    gr = torch.randn(n, device=dev, generator=g) * 1e-3
    m, v, mb = (torch.zeros(n, device=dev) for _ in range(3))
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    shadow = [(0, n, sh, 1, 0, 0, 0)]
    plan, partials, ticket, sums, trust = lamb_opt._workspace(C)
    state = lambda: torch.zeros(4, dtype=torch.int32, device=dev)
    lsched = (lamb_coef_table(1e-6).to(dev), state())
    asched = (coef_table(1e-6).to(dev), state())
    variants = {
        "adamw": lambda: C.adamw(p, gr, m, v, 0.9, 0.999, 1e-8, False, True, shadow, None, asched),
        "lamb_moments": lambda: C.lamb_moments(p, gr, m, v, 0.9, 0.999, 1e-6, False, plan, partials, ticket, sums,
                                               trust, None, lsched),
        "lamb_apply": lambda: C.lamb(p, m, v, 1e-6, True, shadow, plan, trust, lsched),
        "seg_sqnorm": lambda: C.seg_sqnorm(p, gr, plan, partials, ticket, sums, trust, 1e-3, 1e-8, None),
        "lars": lambda: C.lars(p, gr, mb, 1e-6, 0.9, 0.0, False, False, False, True, shadow, plan, trust, None, None),
        "noop": lambda: C.noop(2048),
    }
    us = {k: [] for k in variants}
    for _ in range(a.rounds):  # alternate: every variant once per round
        for k, fn in variants.items():
            us[k].append(timed(fn, a.reps, a.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    for k, v in us.items():
        emit({"bench": "kernel", "name": k, "n": n, "us": med[k], "us_rounds": v})
    pair = med["lamb_moments"] + med["lamb_apply"]
    emit({"bench": "kernel", "name": "lamb pair", "us": pair, "over_adamw": pair / med["adamw"],
          "over_lars_pair": pair / (med["seg_sqnorm"] + med["lars"]), "bytes_ratio_adamw": 42 / 30,
          "gb_per_s_moments": 24 * n / med["lamb_moments"] / 1e3, "gb_per_s_apply": 18 * n / med["lamb_apply"] / 1e3,
          "gb_per_s_adamw": 30 * n / med["adamw"] / 1e3})
    emit({"bench": "kernel", "name": "table", "tensors": plan[0].shape[0], "work_items": plan[1].shape[0],
          "seg_sqnorm_blocks": C.seg_sqnorm_blocks(plan[1].shape[0])})


def step_times(a, emit):
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedAdamW, FusedLAMB

    dev = torch.device("cuda", 0)
    B = a.batch
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)

    def make(kind):
        torch.manual_seed(0)
        model = resnet18(num_classes=1000).to(dev)
        opt = (FusedAdamW if kind == "adamw" else FusedLAMB)(model, lr=1e-3, weight_decay=0.01)
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return GraphedStep(step, (x, y), warmup=2), opt

    runs = {"adamw": make("adamw"), "lamb": make("lamb")}
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
        if k == "lamb":
            ratios = [t["ratio"] for t in runs[k][1].trust_stats().values() if t["adapted"]]
            rec["trust_ratio_min"], rec["trust_ratio_max"] = min(ratios), max(ratios)
        emit(rec)
    return runs["lamb"][1]


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
