"""Evaluation throughput on one GPU: the fused inference kernel vs the module path's forward.

    python scripts/eval_bench.py [--batch 1000] [--repeats 10] [--warmup 3] [--out FILE]
    python scripts/eval_bench.py --model resnet18 [--batch 1000] [--repeats 10] [--out FILE]

Evaluates the 10,000-image synthetic test split at eval batch 1000 in bf16 and fp32, both
builds in one call (same GPU, same clocks, alternating): ``fused`` = csrc/kernels/infer.hip
(one launch per batch + the totals kernel, pxt 1 and 2), ``module`` = what the tree could do
before it: the module path's forward under ``no_grad`` (conv1, conv2 and fc kernels that
materialise a1 and a2) with the same argmax / loss epilogue.  Times are device times between
two events on the stream that runs the work, after warm-up, median and min-max of the
repeats; the per-launch kernel time is a back-to-back train of inference launches without
the totals kernel.  One JSON line per configuration.

``--model resnet18``: see :func:`resnet_main` (fused conv + BatchNorm inference vs the unfused
eval-mode forward)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, stream, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def kernels_per_call(fn):
    """Device kernels launched by one call of ``fn`` (torch.profiler), or None if the profiler
    cannot trace this device."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:  # noqa: BLE001
        return None


def resnet_main(a):
    """``--model resnet18``: the fused conv + BatchNorm inference forward (``forward_infer``,
    BatchNorm folded once outside the loop, as ``evaluate_resnet`` does) vs the unfused
    eval-mode forward under ``no_grad`` (conv -> raw y -> bn_apply, the only route before it),
    on 224 x 224 images at batch 32 and at the evaluation's default batch, in one process,
    alternating repeat by repeat after warm-up.  One JSON line per (batch, path) with images/s
    and kernels per batch, and one with the ratio."""
    from ddp_amd.data import DeviceImages, synthetic_imagenet_test
    from ddp_amd.engine.trainer import TrainOptions
    from ddp_amd.models import resnet18

    dev = torch.device("cuda", 0)
    batches = sorted({32, a.batch if a.batch else TrainOptions().eval_batch_size})
    torch.manual_seed(0)
    model = resnet18(num_classes=1000).to(dev)
    imgs, labels = synthetic_imagenet_test(max(batches), 224, 1000)
    data = DeviceImages(imgs, labels, dev)
    stream = torch.cuda.current_stream()
    folded = model.fold_bn()
    recs = []
    for B in batches:
        x, _ = data.gather(torch.arange(B, device=dev))

        def fused(x=x):
            return model.forward_infer(x, folded)

        def unfused(x=x):
            model.eval()
            try:
                with torch.no_grad():
                    return model(x)
            finally:
                model.train()

        runs = {"fused": fused, "unfused": unfused}
        agree = (fused().float() - unfused().float()).abs().max().item()
        kern = {k: kernels_per_call(fn) for k, fn in runs.items()}
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        ms = {k: [] for k in runs}
        for _ in range(a.repeats):  # alternating: both paths see the same clocks
            for k, fn in runs.items():
                ms[k] += timed(fn, stream, 0, 1)
        for k in runs:
            med = statistics.median(ms[k])
            rec = dict(model="resnet18", path=k, batch=B, image_size=224, ms_median=med, ms_min=min(ms[k]),
                       ms_max=max(ms[k]), images_per_sec=B / med * 1e3, kernels_per_batch=kern[k])
            recs.append(rec)
            print(json.dumps(rec), flush=True)
        rec = dict(model="resnet18", batch=B, fused_over_unfused_images_per_sec=statistics.median(ms["unfused"])
                   / statistics.median(ms["fused"]), max_abs_logit_difference=agree)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["simplecnn", "resnet18"], default="simplecnn")
    ap.add_argument("--batch", type=int, default=None,
                    help="evaluation batch (default 1000; resnet18: measured beside batch 32)")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.model == "resnet18":
        return resnet_main(a)
    a.batch = a.batch or 1000
    from ddp_amd.data import DeviceMNIST, load_mnist
    from ddp_amd.engine.evaluation import FusedEvaluator, evaluate_forward, model_operands
    from ddp_amd.models import SimpleCNN

    dev = torch.device("cuda", 0)
    imgs, labels, _ = load_mnist("/nonexistent", "synthetic", split="test")
    data = DeviceMNIST(imgs, labels, dev)
    n = len(data)
    stream = torch.cuda.current_stream()
    recs = []
    for dtype in ("bf16", "fp32"):
        torch.manual_seed(0)
        model = SimpleCNN(compute_dtype=torch.float32 if dtype == "fp32" else torch.bfloat16).to(dev)
        ops = model_operands(model, dtype)
        runs = {"module": lambda: evaluate_forward(model, data, a.batch)}
        evs = {}
        for pxt in (1, 2):
            evs[pxt] = FusedEvaluator(dev, dtype, pxt)
            runs[f"fused_pxt{pxt}"] = lambda e=evs[pxt]: e.run(data, ops, a.batch)
        res = {k: fn() for k, fn in runs.items()}
        for k, fn in runs.items():
            ms = timed(fn, stream, a.warmup, a.repeats)
            rec = dict(dtype=dtype, path=k, images=n, batch=a.batch, ms_median=statistics.median(ms),
                       ms_min=min(ms), ms_max=max(ms), images_per_sec=n / statistics.median(ms) * 1e3,
                       correct=res[k].correct, loss_sum=res[k].loss_sum)
            if k.startswith("fused"):
                ev, B = evs[int(k[-1])], min(a.batch, n)
                out = [torch.empty(B, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.float32)]

                def train(ev=ev, B=B, out=out):
                    for _ in range(20):
                        ev.C.simplecnn_infer(data.images_u8, data.labels_i32, None, 0, B, ops["w1"], ops["b1"],
                                             ops["w2"], ops["b2"], ops["wfc_frag"], ops["bfc"], ev.fc_part,
                                             ev.img_cnt, out[0], out[1], out[2], None, ev.pxt)

                rec["kernel_us_per_launch"] = statistics.median(timed(train, stream, 2, a.repeats)) * 1e3 / 20
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
