"""Held-out evaluation: accuracy and mean loss of SimpleCNN over a ``DeviceMNIST`` split, and
of ResNet-18 (top-1 and top-5) over a ``DeviceImages`` split.

On the GPU the whole forward of an evaluation batch is ONE launch of the fused inference
kernel (csrc/kernels/infer.hip: conv1 recomputed from the uint8 images, MFMA conv2, bias +
ReLU, the fc partials, and a wait-free tail that writes each image's prediction, loss and
whether it is correct - no activation is stored), followed by the one-block totals kernel
that adds the batch into a running (int64 correct, fp64 loss) pair on the device; a split
costs one device-to-host read.  On the CPU, and on the module path, the model's own forward
runs under ``torch.no_grad()`` with the same tie rule and the same result type.

ResNet-18 (:class:`ResNetEvaluator`, :func:`evaluate_resnet`): on the GPU the inference forward
``ResNet.forward_infer`` - every conv + frozen BatchNorm (+ residual) (+ ReLU) one launch with
the affine in the convolution's epilogue (csrc/kernels/conv_infer.h), the BatchNorm vectors
folded once per call - then the one-wave-per-row tail kernel (prediction, loss, top-1 and
top-5 hit per image) and the one-block totals kernel; again one device-to-host read per
split.  ``engine="module"`` and the CPU run the model's own forward in ``eval()`` under
``no_grad`` with the same tie and top-5 rules (the oracle path).  Evaluation only reads the
model: no autograd graph, no gradient, no BatchNorm buffer and none of the training step's
buffers is written, and ``model.training`` is restored.

Sharding: :func:`eval_shard` partitions the split WITHOUT padding (``DistributedSampler`` pads
with duplicates, which would bias the counts), so after :func:`all_reduce_result` the
accuracy is exact and does not depend on the world size for fixed per-image predictions.
"""
from __future__ import annotations

import dataclasses

import torch

from ..data.loader import DeviceMNIST

HW, NCLS = 28 * 28, 10


@dataclasses.dataclass
class EvalResult:
    correct: int
    count: int
    loss_sum: float
    # per-image outputs of THIS rank's images, in the order they were evaluated (device tensors)
    pred: torch.Tensor | None = None     # int32 [count]
    loss: torch.Tensor | None = None     # float32 [count]
    logits: torch.Tensor | None = None   # float32 [count, 10] (only when asked for)
    correct_rows: torch.Tensor | None = None  # int32 [count]: 1 where pred == label
    correct5: int | None = None               # top-5 hits (ResNet evaluation only)
    correct5_rows: torch.Tensor | None = None  # int32 [count]: 1 where the label is in the top 5

    @property
    def accuracy(self) -> float:
        return self.correct / self.count if self.count else float("nan")

    @property
    def top5(self) -> float:
        if self.correct5 is None:
            return float("nan")
        return self.correct5 / self.count if self.count else float("nan")

    @property
    def mean_loss(self) -> float:
        return self.loss_sum / self.count if self.count else float("nan")


def eval_shard(n: int, world: int, rank: int) -> torch.Tensor:
    """Rank ``rank``'s samples of an ``n``-sample split: contiguous, every sample on exactly one
    rank, no padding, shard sizes differing by at most one (the first ``n % world`` ranks hold
    one more)."""
    if world < 1 or not 0 <= rank < world or n < 0:
        raise ValueError(f"eval_shard: bad (n, world, rank) = ({n}, {world}, {rank})")
    base, extra = divmod(n, world)
    start = rank * base + min(rank, extra)
    return torch.arange(start, start + base + (1 if rank < extra else 0), dtype=torch.int64)


def lowest_argmax(logits: torch.Tensor) -> torch.Tensor:
    """Index of each row's maximum, the LOWEST index on ties (the kernel's strict ``>`` scan
    from class 0; a row with a NaN maximum gives 0 there and here)."""
    mx = logits.max(dim=1, keepdim=True).values
    cls = torch.arange(logits.shape[1], device=logits.device).expand_as(logits)
    cand = torch.where(logits == mx, cls, torch.full_like(cls, logits.shape[1]))
    pred = cand.min(dim=1).values
    return torch.where(pred == logits.shape[1], torch.zeros_like(pred), pred)


def all_reduce_result(res: EvalResult) -> EvalResult:
    """Totals over every rank: one all-reduce of [correct, count] (int64) and one of loss_sum
    (fp64) over the job's control plane - CPU tensors under gloo (same-GPU rehearsals
    included), device tensors under nccl.  Per-image outputs stay the rank's own."""
    import torch.distributed as dist

    if not dist.is_initialized() or dist.get_world_size() == 1:
        return res
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    counts = [res.correct, res.count] + ([res.correct5] if res.correct5 is not None else [])
    cc = torch.tensor(counts, dtype=torch.int64, device=dev)
    ls = torch.tensor([res.loss_sum], dtype=torch.float64, device=dev)
    dist.all_reduce(cc)
    dist.all_reduce(ls)
    cc = cc.cpu()
    out = dataclasses.replace(res, correct=int(cc[0]), count=int(cc[1]), loss_sum=float(ls.cpu()[0]))
    return dataclasses.replace(out, correct5=int(cc[2])) if res.correct5 is not None else out


def _check_indices(indices, n: int, device) -> torch.Tensor | None:
    if indices is None:
        return None
    idx = torch.as_tensor(indices)
    if idx.dim() != 1 or idx.dtype.is_floating_point:
        raise ValueError("evaluate: indices must be a 1-d integer tensor")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise ValueError(f"evaluate: indices must lie in [0, {n})")
    return idx.to(device)


class FusedEvaluator:
    """The fused inference kernel's scratch (partial logits, per-image tickets, the running
    totals) and its launch loop.  The scratch belongs to the evaluator - none of the training
    engine's buffers is touched - and is reused by every call (each launch re-arms its
    tickets); one evaluator runs on one stream at a time."""

    def __init__(self, device, dtype: str = "bf16", pxt: int = 2):
        from .. import native

        self.C = native.require()
        if dtype not in ("bf16", "fp32"):
            raise ValueError(f"evaluate: dtype must be bf16 or fp32, got {dtype!r}")
        if pxt not in (1, 2):
            raise ValueError("evaluate: pxt must be 1 or 2")
        self.device, self.dtype, self.pxt = torch.device(device), dtype, int(pxt)
        self.max_batch = 0
        self.fc_part = self.img_cnt = None
        self.tot_correct = self.tot_loss = None

    def _scratch(self, B: int):
        if self.tot_correct is None:
            self.tot_correct = torch.zeros(1, dtype=torch.int64, device=self.device)
            self.tot_loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        if B > self.max_batch:
            self.fc_part = torch.empty(2 * self.C.infer_blocks(B, self.pxt) * NCLS, dtype=torch.float32,
                                       device=self.device)
            self.img_cnt = torch.zeros(B * self.C.INFER_CNT_STRIDE, dtype=torch.int32, device=self.device)
            self.max_batch = B

    def run(self, data: DeviceMNIST, ops: dict, batch_size: int = 1000, indices=None,
            want_logits: bool = False) -> EvalResult:
        """Evaluate rows ``indices`` (default: all) of ``data`` on the CURRENT stream.  ``ops``:
        w1, b1, w2 (OHWI, bf16 or fp32), b2, wfc_frag (FCFRAG order, same dtype), bfc."""
        if data.device != self.device:
            raise ValueError(f"evaluate: the split lives on {data.device}, the evaluator on {self.device}")
        B = int(batch_size)
        if B < 1 or B * HW >= 2 ** 31:
            raise ValueError("evaluate: need 0 < batch_size * 784 < 2^31")
        idx = _check_indices(indices, len(data), self.device)
        n = len(data) if idx is None else idx.numel()
        i32 = None if idx is None else idx.to(torch.int32).contiguous()
        want = torch.bfloat16 if self.dtype == "bf16" else torch.float32
        if ops["w2"].dtype != want or ops["wfc_frag"].dtype != want:
            raise ValueError(f"evaluate: {self.dtype} operands expected, got {ops['w2'].dtype} / {ops['wfc_frag'].dtype}")
        dev = self.device
        pred = torch.empty(n, dtype=torch.int32, device=dev)
        correct = torch.empty(n, dtype=torch.int32, device=dev)
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        logits = torch.empty(n, NCLS, dtype=torch.float32, device=dev) if want_logits else None
        if n == 0:
            return EvalResult(0, 0, 0.0, pred, loss, logits, correct)
        self._scratch(min(B, n))
        self.tot_correct.zero_()
        self.tot_loss.zero_()
        for s in range(0, n, B):  # (the last batch may be ragged)
            b = min(B, n - s)
            self.C.simplecnn_infer(data.images_u8, data.labels_i32, i32, s, b, ops["w1"], ops["b1"], ops["w2"],
                                   ops["b2"], ops["wfc_frag"], ops["bfc"], self.fc_part, self.img_cnt, pred[s:],
                                   correct[s:], loss[s:], None if logits is None else logits[s:], self.pxt)
            self.C.infer_totals(correct[s:], loss[s:], b, self.tot_correct, self.tot_loss)
        c, ls = int(self.tot_correct.cpu()[0]), float(self.tot_loss.cpu()[0])  # (one wait for the split)
        return EvalResult(c, n, ls, pred, loss, logits, correct)


def model_operands(model, dtype: str = "bf16") -> dict:
    """The inference kernel's operands from a bare SimpleCNN's parameters (checkpoints,
    ``--eval_only``): conv2's OHWI weight and the fc weight in the FCFRAG order, in bf16 (the
    shadows' round-to-nearest-even) or fp32."""
    from ..ops.functional import fc_weight_frag

    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    f = lambda p: p.detach().float().contiguous()  # noqa: E731
    return dict(w1=f(model.net[0].weight).view(-1), b1=f(model.net[0].bias),
                w2=f(model.net[2].weight).to(dt).contiguous(), b2=f(model.net[2].bias),
                wfc_frag=fc_weight_frag(f(model.fl.weight), HW, 64, dt), bfc=f(model.fl.bias))


def evaluate_forward(model, data: DeviceMNIST, batch_size: int = 1000, indices=None,
                     want_logits: bool = False) -> EvalResult:
    """The model's own forward under ``no_grad`` (CPU, and the GPU module path), per batch."""
    dev = data.device
    idx = _check_indices(indices, len(data), dev)
    if idx is None:
        idx = torch.arange(len(data), device=dev)
    n = idx.numel()
    preds, losses, lgs = [], [], []
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for s in range(0, n, int(batch_size)):
                x, y = data.gather(idx[s:s + int(batch_size)])
                lg = model(x).float()
                preds.append(lowest_argmax(lg).to(torch.int32))
                losses.append(torch.logsumexp(lg, dim=1) - lg.gather(1, y.view(-1, 1))[:, 0])
                if want_logits:
                    lgs.append(lg)
    finally:
        model.train(was_training)
    pred = torch.cat(preds) if preds else torch.empty(0, dtype=torch.int32, device=dev)
    loss = torch.cat(losses) if losses else torch.empty(0, dtype=torch.float32, device=dev)
    labels = data.labels_i32.index_select(0, idx)
    rows = (pred == labels).to(torch.int32)
    correct = int(rows.sum())
    loss_sum = float(loss.double().cpu().cumsum(0)[-1]) if n else 0.0  # fp64, index order
    return EvalResult(correct, n, loss_sum, pred, loss, torch.cat(lgs) if lgs else None, rows)


def evaluate(model, data: DeviceMNIST, device=None, dtype: str = "bf16", batch_size: int = 1000,
             indices=None, engine: str = "fused", pxt: int = 2, want_logits: bool = False) -> EvalResult:
    """Evaluate a bare ``SimpleCNN`` (a checkpoint, ``--eval_only``) on rows ``indices`` of
    ``data``: on a GPU with ``engine="fused"`` the fused inference kernel with operands built
    from the model's parameters; on the CPU and with ``engine="module"`` the model's forward."""
    device = torch.device(device) if device is not None else data.device
    if engine not in ("fused", "module"):
        raise ValueError(f"evaluate: engine must be fused or module, got {engine!r}")
    if device.type != "cuda" or engine == "module":
        return evaluate_forward(model, data, batch_size, indices, want_logits)
    ev = FusedEvaluator(device, dtype, pxt)
    with torch.cuda.device(device):
        return ev.run(data, model_operands(model, dtype), batch_size, indices, want_logits)


# ---------------------------------------------------------------------------- ResNet-18
def top5_hit(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """int32 [B]: 1 iff fewer than 5 classes ``j`` rank before the label - ``row[j] > row[label]``,
    or ``row[j] == row[label]`` with ``j < label`` (the tail kernel's rule; with at most 5
    classes every finite row is a hit)."""
    xl = logits.gather(1, labels.view(-1, 1))
    cls = torch.arange(logits.shape[1], device=logits.device).expand_as(logits)
    before = (logits > xl) | ((logits == xl) & (cls < labels.view(-1, 1)))
    return (before.sum(dim=1) < 5).to(torch.int32)


def _check_activation_sizes(model, batch: int, size_hw):
    """The kernels index pixels (and the reduction's elements) with ``int``: refuse a batch
    any of whose activations would reach 2^31 elements (the stem's output is the largest)."""
    h, w = int(size_hw[0]), int(size_hw[1])
    oh, ow = (h + 2 * 3 - 7) // 2 + 1, (w + 2 * 3 - 7) // 2 + 1
    biggest = max(batch * h * w * 4, batch * oh * ow * model.conv1.out_channels)
    if biggest >= 2 ** 31:
        raise ValueError(f"evaluate_resnet: a batch of {batch} {h}x{w} images has an activation of {biggest} "
                         f">= 2^31 elements; lower the evaluation batch size")


class ResNetEvaluator:
    """The ResNet inference path's running totals (int64 [top-1, top-5], fp64 loss) and its
    launch loop.  Nothing of the training step is shared: outputs and totals belong to the
    evaluator, the model is only read."""

    def __init__(self, device):
        from .. import native

        self.C = native.require()
        self.device = torch.device(device)
        self.tot = self.tot_loss = None

    def run(self, model, data, batch_size: int = 256, indices=None, want_logits: bool = False) -> EvalResult:
        """Evaluate rows ``indices`` (default: all) of the ``DeviceImages`` split on the CURRENT
        stream."""
        if data.device != self.device:
            raise ValueError(f"evaluate: the split lives on {data.device}, the evaluator on {self.device}")
        B = int(batch_size)
        if B < 1:
            raise ValueError("evaluate_resnet: batch_size must be >= 1")
        idx = _check_indices(indices, len(data), self.device)
        if idx is None:
            idx = torch.arange(len(data), device=self.device)
        idx = idx.to(torch.int64).contiguous()
        n = idx.numel()
        _check_activation_sizes(model, min(B, max(n, 1)), data.images_u8.shape[1:3])
        dev = self.device
        ncls = model.fc.weight.shape[0]
        pred = torch.empty(n, dtype=torch.int32, device=dev)
        correct = torch.empty(n, dtype=torch.int32, device=dev)
        correct5 = torch.empty(n, dtype=torch.int32, device=dev)
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        logits = torch.empty(n, ncls, dtype=torch.float32, device=dev) if want_logits else None
        if n == 0:
            return EvalResult(0, 0, 0.0, pred, loss, logits, correct, 0, correct5)
        if self.tot is None:
            self.tot = torch.zeros(2, dtype=torch.int64, device=dev)
            self.tot_loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.tot.zero_()
        self.tot_loss.zero_()
        was_training = model.training
        try:
            with torch.no_grad():
                folded = model.fold_bn()  # once per evaluation call
                for s in range(0, n, B):  # (the last batch may be ragged)
                    b = min(B, n - s)
                    x, y = data.gather(idx[s:s + b])
                    lg = model.forward_infer(x, folded)
                    self.C.resnet_eval_tail(lg, y, pred[s:], loss[s:], correct[s:], correct5[s:])
                    self.C.resnet_eval_totals(correct[s:], correct5[s:], loss[s:], b, self.tot, self.tot_loss)
                    if logits is not None:
                        logits[s:s + b] = lg
        finally:
            model.train(was_training)
        tot, ls = self.tot.cpu(), float(self.tot_loss.cpu()[0])  # (the split's only waits)
        return EvalResult(int(tot[0]), n, ls, pred, loss, logits, correct, int(tot[1]), correct5)


def evaluate_resnet_forward(model, data, batch_size: int = 256, indices=None,
                            want_logits: bool = False) -> EvalResult:
    """The model's own forward in ``eval()`` under ``no_grad`` (CPU, and the GPU module path),
    per batch, with the tail kernel's tie and top-5 rules in torch."""
    dev = data.device
    idx = _check_indices(indices, len(data), dev)
    if idx is None:
        idx = torch.arange(len(data), device=dev)
    idx = idx.to(torch.int64)
    n = idx.numel()
    B = int(batch_size)
    if B < 1:
        raise ValueError("evaluate_resnet: batch_size must be >= 1")
    _check_activation_sizes(model, min(B, max(n, 1)), data.images_u8.shape[1:3])
    preds, losses, lgs, hits5 = [], [], [], []
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for s in range(0, n, B):
                x, y = data.gather(idx[s:s + B])
                lg = model(x).float()
                preds.append(lowest_argmax(lg).to(torch.int32))
                losses.append(torch.logsumexp(lg, dim=1) - lg.gather(1, y.view(-1, 1))[:, 0])
                hits5.append(top5_hit(lg, y))
                if want_logits:
                    lgs.append(lg)
    finally:
        model.train(was_training)
    pred = torch.cat(preds) if preds else torch.empty(0, dtype=torch.int32, device=dev)
    loss = torch.cat(losses) if losses else torch.empty(0, dtype=torch.float32, device=dev)
    rows5 = torch.cat(hits5) if hits5 else torch.empty(0, dtype=torch.int32, device=dev)
    labels = data.labels.index_select(0, idx)
    rows = (pred == labels).to(torch.int32)
    loss_sum = float(loss.double().cpu().cumsum(0)[-1]) if n else 0.0  # fp64, index order
    return EvalResult(int(rows.sum()), n, loss_sum, pred, loss, torch.cat(lgs) if lgs else None, rows,
                      int(rows5.sum()), rows5)


def evaluate_resnet(model, data, device=None, batch_size: int = 256, indices=None, engine: str = "fused",
                    want_logits: bool = False) -> EvalResult:
    """Evaluate a ResNet on rows ``indices`` of a ``DeviceImages`` split: on a GPU with
    ``engine="fused"`` the fused conv + BatchNorm inference path; on the CPU and with
    ``engine="module"`` the model's own forward in ``eval()``."""
    device = torch.device(device) if device is not None else data.device
    if engine not in ("fused", "module"):
        raise ValueError(f"evaluate_resnet: engine must be fused or module, got {engine!r}")
    if device.type != "cuda" or engine == "module":
        return evaluate_resnet_forward(model, data, batch_size, indices, want_logits)
    with torch.cuda.device(device):
        return ResNetEvaluator(device).run(model, data, batch_size, indices, want_logits)
