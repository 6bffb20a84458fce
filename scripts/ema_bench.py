"""Cost of the weight EMA (WeightEMA, ema_kernel / ema_swap_kernel), measured in ONE call (same
process, same clocks, alternating rounds):

* the bare ``ema_kernel<false>`` (decay by value), ``ema_kernel<true>`` (decay table + tickets)
  and ``ema_swap_kernel`` (with the bf16 shadow) at ResNet-18's flat parameter count, beside
  ``sgd_kernel`` with momentum 0.9 by value and its DLR build (the same ticket protocol) -
  in-graph time per launch as scripts/kbench.py measures it;
* the ResNet-18 graphed training step (batch 32, 224 x 224) with ``FusedSGD(momentum=0.9)``:
  without an EMA, with a constant-decay EMA and with a warm-up EMA attached.

    python scripts/ema_bench.py [--reps 20] [--iters 10] [--rounds 5] [--steps 20] [--json out.jsonl]
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
from ddp_amd.ops.ema import warmup_table  # noqa: E402
from kbench import timed  # noqa: E402  (scripts/ is sys.path[0] when run as a script)


def kernel_times(C, n, a, emit):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    gr = torch.randn(n, device=dev, generator=g) * 1e-3
    mb = torch.zeros(n, device=dev)
    e = p.clone()
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    table = torch.full((1000,), 1e-6, device=dev)
    etab = warmup_table(0.9999).to(dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    cstate = torch.zeros(4, dtype=torch.int32, device=dev)
    wstate = torch.zeros(4, dtype=torch.int32, device=dev)
    shadow = [(0, n, sh, 1, 0, 0, 0)]

    def sgd(sched):
        return lambda: C.sgd(p, gr, mb, 1e-6, 0.9, 0.0, 0.0, False, False, False, True, shadow, None, sched)

    variants = {
        "sgd momentum by value": sgd(None),
        "sgd momentum DLR": sgd((table, state)),
        "ema constant": lambda: C.ema(e, p, 1e-4, cstate, None),
        "ema warmup": lambda: C.ema(e, p, 1e-4, wstate, etab),
        "ema swap": lambda: C.ema_swap(p, e, shadow),
        "noop": lambda: C.noop(2048),
    }
    us = {k: [] for k in variants}
    for _ in range(a.rounds):  # alternate: every variant once per round
        for k, fn in variants.items():
            us[k].append(timed(fn, a.reps, a.iters))
    for k, v in us.items():
        emit({"bench": "kernel", "name": k, "n": n, "us": statistics.median(v), "us_rounds": v})
    emit({"bench": "kernel", "name": "ema state", "constant": cstate.cpu().tolist()[:2], "warmup": wstate.cpu().tolist()[:2]})
    # bytes per element: sgd reads p, g, m and writes p, m (+ 2-byte shadow); the EMA reads e, p and
    # writes e; the swap reads and writes both (+ shadow)
    emit({"bench": "kernel", "name": "bytes", "sgd_bytes_per_elem": 22, "ema_bytes_per_elem": 12,
          "swap_bytes_per_elem": 18, "ema_byte_ratio": 12 / 22, "swap_byte_ratio": 18 / 22})


def step_times(a, emit):
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD, WeightEMA

    dev = torch.device("cuda", 0)
    B = a.batch
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)

    def make(kind):
        torch.manual_seed(0)
        model = resnet18(num_classes=1000).to(dev)
        opt = FusedSGD(model, lr=0.01, momentum=0.9)
        ema = None
        if kind != "no ema":
            ema = WeightEMA(model, decay=0.9999, warmup=kind == "ema warmup")
            opt.attach_ema(ema)
        lossf = CrossEntropyLoss()

        def step(x, y):
            opt.zero_grad()
            loss = lossf(model(x), y)
            loss.backward()
            opt.step()
            return loss
        return GraphedStep(step, (x, y), warmup=2), opt, ema

    runs = {k: make(k) for k in ("no ema", "ema constant", "ema warmup")}
    ips = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (gs, _, _) in runs.items():
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
        if runs[k][2] is not None:
            rec["ema_updates"], rec["expected_updates"] = runs[k][2].num_updates(), 2 + a.rounds * (a.steps + 1)
        emit(rec)
    # the exchange and back, as --eval_ema pays it around every evaluation
    ema = runs["ema constant"][2]
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        with ema.applied():
            pass
        torch.cuda.synchronize()
        ts.append(1e6 * (time.perf_counter() - t0))
    emit({"bench": "applied() enter + exit, wall", "us": statistics.median(ts), "us_rounds": ts})
    return runs["no ema"][1].flat.numel


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
