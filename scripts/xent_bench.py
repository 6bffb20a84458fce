"""Cost of label smoothing (CrossEntropyLoss(label_smoothing=), the SMOOTH builds of the
cross-entropy kernels), measured in ONE call with alternating rounds:

* the bare ``xent_wave_rows_kernel`` without and with smoothing at B = 32, C = 1000 (and
  ``xent_kernel`` at B = 32, C = 10) - in-graph time per launch as scripts/kbench.py measures
  it, beside an empty launch;
* the ResNet-18 graphed training step (batch 32, 224 x 224, FusedSGD momentum 0.9) with
  ``label_smoothing`` 0 and 0.1 on this build and, with ``--parent_so PATH`` (a ``_C.so`` built
  from the parent commit), with 0 on that build.  Every variant of a round is a fresh child
  process of this script (``--child``: one build per process; the variants alternate, so clock
  and thermal drift hits them alike).

    python scripts/xent_bench.py [--rounds 3] [--steps 50] [--parent_so variants/parent/_C.so] [--json out.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def kernel_times(a, emit):
    from ddp_amd import native
    from kbench import timed  # (scripts/ is sys.path[0] when run as a script)

    C = native.require()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)

    def case(B, NC):
        lg = torch.randn(B, NC, device=dev, generator=g) * 3
        lab = torch.randint(0, NC, (B,), device=dev, generator=g)
        dl, loss = torch.empty_like(lg), torch.empty(1, device=dev)
        return lambda eps: (lambda: C.xent(lg, 1, None, lab, None, dl, loss, None, 1.0 / B, 0.0, label_smoothing=eps))

    wave, block = case(32, 1000), case(32, 10)
    variants = {"wave rows 32x1000 plain": wave(0.0), "wave rows 32x1000 SMOOTH": wave(0.1),
                "block 32x10 plain": block(0.0), "block 32x10 SMOOTH": block(0.1), "noop": lambda: C.noop(8)}
    us = {k: [] for k in variants}
    for _ in range(a.kernel_rounds):  # alternate: every variant once per round
        for k, fn in variants.items():
            us[k].append(timed(fn, a.reps, a.iters))
    for k, v in us.items():
        emit({"bench": "kernel", "name": k, "us": statistics.median(v), "us_rounds": v})


def child(a):
    """One build, one label_smoothing: capture the step, time ``steps`` replays, print one JSON line."""
    from ddp_amd.engine import GraphedStep
    from ddp_amd.models import resnet18
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    dev = torch.device("cuda", 0)
    B = a.batch
    torch.manual_seed(0)
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)
    model = resnet18(num_classes=1000).to(dev)
    opt = FusedSGD(model, lr=0.01, momentum=0.9)
    lossf = CrossEntropyLoss(label_smoothing=a.child)

    def step(x, y):
        opt.zero_grad()
        loss = lossf(model(x), y)
        loss.backward()
        opt.step()
        return loss

    gs = GraphedStep(step, (x, y), warmup=2)
    for _ in range(a.warmup):
        gs(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = gs(x, y)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"img_per_s": a.steps * B / dt, "ms_per_step": 1e3 * dt / a.steps, "loss": loss.item()}), flush=True)


def step_times(a, emit):
    runs = {"eps=0 this build": (0.0, None), "eps=0.1 this build": (0.1, None)}
    if a.parent_so:
        runs = {"eps=0 this build": (0.0, None), "eps=0 parent build": (0.0, os.path.abspath(a.parent_so)),
                "eps=0.1 this build": (0.1, None)}
    res = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (eps, so) in runs.items():
            env = dict(os.environ)
            if so:
                env["DDP_AMD_NATIVE_SO"] = so
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(eps), "--steps", str(a.steps),
                                "--warmup", str(a.warmup), "--batch", str(a.batch)], env=env, stdout=subprocess.PIPE,
                               text=True, timeout=a.child_timeout)
            if p.returncode != 0:  # a failed child ends the measurement: nothing more is started
                raise SystemExit(f"{k}: child exited with {p.returncode}")
            res[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
    for k, v in res.items():
        ips = [r["img_per_s"] for r in v]
        emit({"bench": "resnet18 graphed step", "name": k, "batch": a.batch, "img_per_s": statistics.median(ips),
              "img_per_s_rounds": ips, "ms_per_step": 1e3 * a.batch / statistics.median(ips), "loss": v[-1]["loss"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kernel_rounds", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--parent_so", default=None, help="a _C.so built from the parent commit (A/B at eps = 0)")
    ap.add_argument("--child_timeout", type=float, default=150.0)
    ap.add_argument("--child", type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    out = open(a.json, "a") if a.json else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    step_times(a, emit)  # the children first: this process has not opened the GPU yet
    kernel_times(a, emit)


if __name__ == "__main__":
    main()
