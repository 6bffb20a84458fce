"""ResNet-50's pointwise layers, new route against the parent route, and the whole step.

For every distinct 1x1 / s1 layer shape of ResNet-50 (batch B, SIDE x SIDE images):

* forward: ``conv_pw_fwd`` (training epilogue; the deferred BatchNorm + ReLU applied while
  staging where the layer's input is deferred) against the parent route on the same tensors -
  ``conv_gemm_fwd`` on the gathered plan, plus the ``bn_apply`` pass in front of it where the
  input is deferred;
* weight gradient: ``conv_pw_wgrad`` against ``conv_gemm_wgrad`` (both with their slab +
  ``grad_reduce`` when they chunk; the parent also pays the deferred layers' ``bn_apply`` in the
  forward only, so none is charged here).

Each route's REPS launches are captured in one graph (device-bound, no host gaps) and the two
graphs are replayed alternately for ROUNDS rounds; a row reports the median time per launch of
each route and ``spread`` = the largest (max - min) / median either route shows over its own
rounds - a difference inside it is not a difference.  ``--step`` times the graphed training step
of ``--model`` instead (img/s), ``--tiles`` adds every forced tile of the new kernels.

    python scripts/resnet50_bench.py [--batch 32] [--side 224] [--tiles]
    python scripts/resnet50_bench.py --step --model resnet50 [--steps 30]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ddp_amd import native  # noqa: E402

BF = torch.bfloat16
dev = "cuda"


def layers(side):
    """(name, Cin, Cout, H, deferred input) of ResNet-50's distinct pointwise layers."""
    h = side // 4
    out = [("l1.conv1.first", 64, 64, h, False), ("l1.downsample", 64, 256, h, False)]
    for i, w in enumerate((64, 128, 256, 512)):
        hi = h >> i
        if i:
            out.append((f"l{i + 1}.conv1.first", 2 * w, w, 2 * hi, False))  # the stride is on conv2
        out += [(f"l{i + 1}.conv1", 4 * w, w, hi, False), (f"l{i + 1}.conv3", w, 4 * w, hi, True)]
    return out


def timed(graphs, rounds):
    """Median ms per replay of each graph and the worst relative spread, replayed alternately."""
    ts = [[] for _ in graphs]
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for g, t in zip(graphs, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    med = [statistics.median(t) for t in ts]
    return med, max((max(t) - min(t)) / m for t, m in zip(ts, med))


def capture(fn, reps):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(reps):
            fn()
    return g


def layer_rows(a):
    C = native.require()
    gen = torch.Generator().manual_seed(0)
    for name, Cin, Cout, H, deferred in layers(a.side):
        N, P = a.batch, a.batch * H * H
        x = torch.randn(N, H, H, Cin, generator=gen).to(BF).to(dev)
        w = (torch.randn(Cout, 1, 1, Cin, generator=gen) * 0.05).to(BF).to(dev)
        dy = torch.randn(N, H, H, Cout, generator=gen).to(BF).to(dev)
        y, xm = torch.empty_like(dy), torch.empty_like(x)
        bn = [torch.randn(Cin, device=dev) * 0.1, torch.rand(Cin, device=dev) + 0.5, torch.ones(Cin, device=dev),
              torch.zeros(Cin, device=dev)] if deferred else None
        _, _, splits, rows, _, _ = C.conv_gemm_plan(x, y, 1, 1, 1, 0)
        st_old = torch.empty(rows, 2, Cout, device=dev)
        part = torch.empty(splits * P * Cout, device=dev) if splits > 1 else None
        _, bp, bc, _ = C.conv_pw_plan(P, Cin, Cout)
        st_new = torch.empty(-(-P // 64), 2, Cout, device=dev)  # rows of the narrowest pixel tile: any plan fits

        def old_fwd():
            src = x
            if deferred:
                C.bn_apply(x, bn[0], bn[1], bn[2], bn[3], None, True, xm)
                src = xm
            C.conv_gemm_fwd(src, w, None, y, 1, 1, 1, 0, False, st_old, part)

        def new_fwd(bp=0, bc=0):
            C.conv_pw_fwd(x, w, y, st_new, bn, bp, bc)

        dw = torch.empty(Cout * Cin, device=dev)
        ppc = C.conv_gemm_wgrad_ppc(x, dy, 1, 1, 1, 0)
        ch_old = C.conv_gemm_wgrad_chunks(x, dy, 1, 1, 1, 0, ppc)
        slab_old = torch.empty(ch_old, Cout * Cin, device=dev)

        def old_wgrad():
            if ch_old == 1:
                C.conv_gemm_wgrad(dy, x, dw, 1, 1, 1, 0, ppc, False)
            else:
                C.conv_gemm_wgrad(dy, x, slab_old, 1, 1, 1, 0, ppc, False)
                C.grad_reduce([(slab_old, Cout * Cin, 0, Cout * Cin, ch_old, dw, 1.0, False)])

        def new_wgrad(bm=0, bnt=0):
            ch = C.conv_pw_wgrad_plan(P, Cin, Cout, bm, bnt, 0)[3]
            if ch == 1:
                C.conv_pw_wgrad(dy, x, dw, False, bn, bm, bnt, 0)
            else:
                if ch not in slabs:
                    slabs[ch] = torch.empty(ch, Cout * Cin, device=dev)
                slab = slabs[ch]
                C.conv_pw_wgrad(dy, x, slab, False, bn, bm, bnt, 0)
                C.grad_reduce([(slab, Cout * Cin, 0, Cout * Cin, ch, dw, 1.0, False)])

        slabs = {}
        flops = 2.0 * P * Cin * Cout
        for op, old, new in (("fwd", old_fwd, new_fwd), ("wgrad", old_wgrad, new_wgrad)):
            routes = {"parent": old, "pw": new}
            if a.tiles:
                for t in ((128, 128), (128, 64), (64, 64)):
                    if Cout % t[0 if op == "wgrad" else 1] == 0 and (op == "fwd" or Cin % t[1] == 0):
                        routes[f"pw{t[0]}x{t[1]}"] = (lambda t=t, new=new: new(*t))
            med, spread = timed([capture(f, a.reps) for f in routes.values()], a.rounds)
            row = dict(layer=name, op=op, Cin=Cin, Cout=Cout, P=P, deferred=deferred, spread=round(spread, 4),
                       plan=dict(fwd=(bp, bc), wgrad=tuple(C.conv_pw_wgrad_plan(P, Cin, Cout)))[op])
            for k, m in zip(routes, med):
                row[k + "_us"] = round(1e3 * m / a.reps, 2)
            row["pw_tflops"] = round(flops / (row["pw_us"] * 1e-6) / 1e12, 1)
            row["ratio"] = round(row["pw_us"] / row["parent_us"], 3)
            print(json.dumps(row), flush=True)


def step_rate(a):
    from ddp_amd import models
    from ddp_amd.engine import GraphedStep
    from ddp_amd.ops import CrossEntropyLoss, FusedSGD

    torch.manual_seed(0)
    model = getattr(models, a.model)(num_classes=1000).to(dev)
    opt, lossf = FusedSGD(model, lr=0.05, momentum=0.9, weight_decay=1e-4), CrossEntropyLoss()
    x = torch.randn(a.batch, a.side, a.side, 4, device=dev).to(BF)
    x[..., 3] = 0
    y = torch.randint(0, 1000, (a.batch,), device=dev)

    def step(xi, yi):
        opt.zero_grad()
        loss = lossf(model(xi), yi)
        loss.backward()
        opt.step()
        return loss

    gs = GraphedStep(step, (x, y), warmup=3)
    rates = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            gs(x, y)
        t1.record()
        t1.synchronize()
        rates.append(a.batch * a.steps / (t0.elapsed_time(t1) * 1e-3))
    print(json.dumps(dict(model=a.model, batch=a.batch, side=a.side, img_per_s=round(statistics.median(rates), 1),
                          min=round(min(rates), 1), max=round(max(rates), 1))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tiles", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    step_rate(a) if a.step else layer_rows(a)
