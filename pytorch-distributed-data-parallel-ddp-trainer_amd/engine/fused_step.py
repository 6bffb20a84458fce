"""Python driver of the native fused SimpleCNN step engine (csrc/runtime/engine.cpp).

The engine trains the SAME parameters as the ``SimpleCNN`` module (its flat fp32
buffer is the engine's parameter buffer), so ``state_dict()`` / checkpoints /
resume work unchanged; only the step itself is replaced by 2 fused HIP kernels
(default fuse level 3: the conv forward, which also produces dZ2 and dL; then the conv
backward with the fused slab reduction + SGD, whose launch also runs the fc weight
gradient + SGD as a third role) - at world size > 1 the fc weight gradient is a light
kernel of its own between the two, so that its bucket's all-reduce (direct xGMI kernels,
or RCCL) overlaps the conv backward - captured into one hipGraph per ``graph_steps``
steps.

Per epoch: the rank's ``DistributedSampler``-exact index list is uploaded once
(int32, into a fixed device buffer the graph reads through a device step
counter), full batches replay the graph, the leftover full steps and the ragged
last batch (drop_last=False) run eagerly with their real size.  Losses are
written on device into a per-epoch history; the host reads them one chunk
behind the GPU (a chunk = one replay), so logging never stalls the stream.
"""
from __future__ import annotations

import dataclasses
import os
import math

import torch

from .. import native
from ..data.loader import DeviceMNIST
from ..data.sampler import ShardedSampler
from ..models.layers import flat_space
from ..ops.functional import wgrad_rows
from ..parallel.ddp import bucket_plan, bucket_ranges

# buckets up to this many fp32 elements may get a one-shot xGMI channel: the bucket must
# fit one kernel grid (1024 x 256); below it the cost model's crossover decides
# (parallel/bucket_model.py: SimpleCNN's 75 KB conv bucket is one-shot at every N; the
# 2 MB fc bucket (501,770 elements) is above this cap, so it is always two-shot).  The
# module path (ddp.py), the planner and describe() use the same cap.
from ..parallel.bucket_model import ONESHOT_MAX_ELEMS  # noqa: E402

BF16 = torch.bfloat16


@dataclasses.dataclass
class EngineOptions:
    graph_steps: int = 100     # steps per captured graph (one loss readback per chunk)
    use_graph: bool = True
    # forward pixel tiles per wave: 1 = 256-thread blocks, 2 = 512-thread blocks.  None: 1 for
    # bf16 when its level-3 grid fits the GPU at once (B <= ~41: the step head's forward, and
    # equal in-call / +1 % driver-shaped at B = 32, profiles/r5_pxt_fwd), else 2 (bf16 B = 64:
    # the OCC 2 forward; exact fp32).  The two group the fc partial logits differently, so
    # chains compared bit for bit must run the same value.
    pxt_fwd: int | None = None
    pxt_dgrad: int = 2
    wgrad_rows: int | None = None
    bucket_cap_mb: float = 25.0
    first_bucket_mb: float = 1.0   # torch DDP's first-bucket cap (the rest use bucket_cap_mb)
    # "model": the xGMI cost model's plan (parallel/bucket_model.engine_plan: one bucket per
    # stage - [fc] then [conv] - which is also the reference DDP's rebuilt layout);
    # "torch": torch's size rule with bucket_cap_mb / first_bucket_mb
    bucket_plan: str = "model"
    force_allreduce: bool = False  # bucket all-reduces even at world size 1 (plumbing tests)
    # 0: 8 kernels/step (a1 stored, separate xent); 1: 6 kernels/step (conv1 recomputed
    # inside conv2 fwd/dgrad/wgrad from the uint8 images, xent folded into fc_bwd; 3 with
    # the fused optimizer and the fused slab reduction: forward -> fc_bwd -> conv backward);
    # (2 - fc_bwd and the conv backward in one launch - measured slower, removed in round 4);
    # 3: the fc backward off the critical path - the forward computes dZ2 itself (per-image
    # in-launch wait for the logits) and the fc weight gradient + SGD runs as a role of the
    # conv backward launch (critical path: forward -> conv backward).  bf16 and fp32, any
    # batch up to 64 (in-order dispatch: a forward block only waits for its own image's
    # blocks, so the grid need not be resident at once - conv3x3_fwd_dz_fits) where the GPU
    # is not shared by several ranks; elsewhere the level-1 chain runs.  Bit-identical to
    # level 1.
    fuse_level: int = 3
    # level 3, single process: the fc weight gradient as a third role of the conv backward
    # launch (2 kernels per step) - 1: its blocks (one 128-column chunk per wave) after every
    # conv block, on the resident slots the conv blocks leave free; 0: its own light kernel
    # between forward and conv backward (what world size > 1 always runs, so the fc bucket's
    # all-reduce overlaps the conv backward)
    l3_fc_role: int = 1
    # single-process steps: SGD in the epilogues of fc_bwd / grad_reduce (no optimizer kernel)
    fuse_opt: bool = True
    # level >= 1: the conv backward launch also reduces the split-K weight-gradient slabs
    # (+ fused SGD) after an in-launch arrival count - no separate grad_reduce kernel
    # 1: slab reduction inside the conv backward while its reducers fit half the launch's
    # resident capacity; 2: the whole capacity when nothing else runs (single process) -
    # lets the exact-fp32 step fuse, measured slower there (385-386k vs 389-391k img/s,
    # profiles/r3_fp32: its 224 waiting reducers hold the CUs the one-block-per-CU dgrad /
    # wgrad roles need); 0: the separate grad_reduce kernel.  None: 1 for bf16, 0 for fp32 -
    # the exact-fp32 level-3 step at two blocks per CU fuses under rule 1 but runs faster
    # with the separate kernel (B = 32: 438k -> 459k img/s in-call, 408k -> 426k driver-
    # shaped; forced dist 362k -> 378k; B = 64 on par; bitwise the same -
    # profiles/r6_rebuilt/fp32_fuse_reduce.md); bf16 keeps the fused one (973k vs 816k), and
    # so does dist_mode 2, whose in-launch all-reduce counts the fused reducers
    fuse_reduce: int | None = None
    # level 1: 0 = the conv backward recomputes conv1 from the compact uint8 batch;
    # 1 = the forward stores a1 and the dgrad role reads its ReLU mask from it; 2 = the
    # wgrad role reads a1 tiles too.  None = 1 for bf16 (with the wgrad role split over
    # channel halves the dgrad role is the conv backward's critical path: 808k -> 825k
    # img/s at B = 32, 1.08M -> 1.11M at B = 64, profiles/r2_split), 0 for fp32
    store_a1: int | None = None
    # bucket all-reduce data plane at world size > 1 (the direct kernels fall back to RCCL
    # when their self-test fails): "auto"/"xgmi" = the direct xGMI kernels, one-shot for
    # buckets <= ONESHOT_MAX_ELEMS (deterministic: same plane on every start, so resumes
    # reduce in the same order); "tune" = time two-shot, two-shot + one-shot and RCCL on
    # the node and keep the fastest; "xgmi2" / "xgmi1" = that plan, forced; "rccl" = RCCL
    comm: str = "auto"
    # copy the rank's samples into epoch order once per epoch (images + labels, one
    # index_select each): the step's batch is then rows [step * B, step * B + B) - one
    # dependent load fewer at the head of every forward (no index-list lookup)
    epoch_order: bool = True
    # compute precision: "bf16" (bf16 MFMA operands, fp32 master weights / gradients /
    # optimizer) or "fp32" (exact fp32 operands on v_mfma_f32_16x16x4_f32 - the
    # reference's precision; the same level-3 / level-1 chains)
    dtype: str = "bf16"
    # fused conv backward: 2 = two wgrad blocks per slab row, one per half of conv2's input
    # channels (half the conv1 recompute and MFMAs on the role's critical path; bit-identical
    # slabs - bf16: 801k -> 811k img/s at B = 32, 1.04M -> 1.06M at B = 64, profiles/r2_split);
    # for fp32 the dgrad role is split the same way (weights read from global) so both roles
    # run at two blocks per CU; 1 = one block per row (fp32: the round-3 kernels, 1 block/CU)
    wgrad_split: int = 2
    # world size > 1, level 3 - how the backward meets the bucket all-reduces (all bitwise
    # equal): 2 = in-launch (xGMI plane): the fc weight gradient is the conv backward's fc
    # role and role blocks at the head of that launch all-reduce each bucket (+ fused SGD) as
    # soon as it is final - 2 kernels per step, as on one GPU (engine.cpp make_xar, conv3x3.hip
    # XAR); 1 = fc_bwd + the fc buckets' all-reduces on a graph branch forked after the
    # forward (schedule_backward); 3 = one stream: the fc role inside the conv backward, the
    # bucket kernels behind it (no cross-stream edge); 0 = the round-4 serial order;
    # 4 = the step head (bf16, xGMI; forces pxt_fwd 1 when the step all-reduces): mode 3's
    # chain, but in a captured graph step k's bucket-pair launch also runs step k + 1's
    # forward (2 launches per step instead of 3; conv3x3.hip step_head_kernel) - same bits as
    # mode 3 at pxt 1.  The default (round 6: forced world 1 751-756k vs mode 3 692-700k
    # img/s, profiles/r6_dist); fp32, the RCCL plane and a head grid that does not fit the
    # GPU run mode 3's launches.  bench.py times the placements on the node at N > 1.
    dist_mode: int = 4
    # dist_mode 2: the most blocks of a bucket's xGMI channel (its role blocks wait at the
    # head of the conv backward grid; the engine takes the in-launch path while the channels'
    # blocks total <= 192).  Forced world 1: 40 -> 479k, 96 -> 535k, 128 -> 525k, 173 -> 499k
    # img/s (profiles/r5_dist); dist_mode 3 698k
    xar_blocks: int = 96
    # bucket plan as for this many ranks (None: the real world size) - forced all-reduces
    # at world size 1 (--force_allreduce) then run the multi-GPU plan's buckets
    plan_world: int | None = None
    # a comm_calibration fit (dict: launch_us, barrier_us, link_eff, topology, ...) measured by
    # this job; the bucket plan and the one-shot choice are made with it
    cost_fit: dict | None = None


def agree(store, key: str, rank: int, world: int, ok: bool) -> bool:
    """True when every rank reported ``ok`` under ``key`` (a c10d store; None = one rank)."""
    if store is None or world <= 1:
        return bool(ok)
    store.set(f"{key}/{rank}", b"1" if ok else b"0")
    return all(store.get(f"{key}/{r}") == b"1" for r in range(world))


# ---------------------------------------------------------------------- reduction oracle
# the start-up check compares the production chain's reduced gradient with a
# sum computed WITHOUT the xGMI code - every rank's local (prescaled) gradient gathered over
# the process group and added in rank order on the host - so a stale or misplaced read in
# the fence-free cross-GPU protocol cannot pass by being shared with the reference chain.

def gather_rank_sum(local: torch.Tensor, world: int) -> torch.Tensor:
    """Every rank's ``local`` (same shape, fp32) summed in rank order 0..world-1 on the host
    (``acc = g0; acc += g1; ...`` - IEEE fp32 adds in the order the xGMI kernels use),
    gathered over the default process group (gloo: host tensors, nccl: device tensors).
    Collective."""
    import torch.distributed as dist

    src = local.detach().float().contiguous()
    if world <= 1 or not dist.is_initialized():
        return src.cpu().clone()
    if dist.get_backend() == "gloo":
        src = src.cpu()
    parts = [torch.empty_like(src) for _ in range(world)]
    dist.all_gather(parts, src)
    acc = parts[0].cpu().clone()
    for p in parts[1:]:
        acc += p.cpu()
    return acc


def oracle_mismatches(reduced: torch.Tensor, oracle: torch.Tensor, ranges) -> int:
    """Elements of the bucket ranges where ``reduced`` differs from ``oracle`` bit for bit."""
    r = reduced.detach().float().cpu().contiguous()
    o = oracle.detach().float().cpu().contiguous()
    bad = 0
    for off, n in ranges:
        bad += int((r[off:off + n].view(torch.int32) != o[off:off + n].view(torch.int32)).sum())
    return bad


# ---------------------------------------------------------------------- placement choice
# at N > 1 the multi-GPU placement (EngineOptions.dist_mode) is timed on the
# node it runs on instead of being fixed by a world-1 measurement.  Only placements that give
# the same bits compete (all of them sum in the plane's fixed order), so the choice never
# changes the trained parameters, only the speed.
PLACEMENT_NAMES = {0: "serial", 1: "fork", 3: "pair", 4: "step head"}


def placement_candidates(comm_kind: str, dtype: str = "bf16") -> tuple:
    """dist_modes worth timing on a data plane: xGMI - the step head (4: the pair launch
    carrying the next step's forward; bf16 only), the pair launch (3), the serial bucket
    kernels (0) and the forked fc branch (1); RCCL - 0 and 1 (its calls never share a launch).
    dist_mode 2 (in-launch) needs the in-order-dispatch opt-in and is not a candidate."""
    if comm_kind.startswith("xgmi"):
        return (4, 3, 0, 1) if dtype == "bf16" else (3, 0, 1)
    if comm_kind.startswith("rccl"):
        return (0, 1)
    return ()


def choose_placement(all_times) -> tuple:
    """``all_times``: every rank's {dist_mode: us per step, or None when it failed there}.  A
    step is as slow as its slowest rank, so each mode counts with its max over ranks; the
    fastest such mode wins (ties: the lower mode).  Returns (mode or None, {mode: max us})."""
    modes = sorted(set().union(*[set(t) for t in all_times]))
    worst = {}
    for m in modes:
        vals = [t.get(m) for t in all_times]
        worst[m] = None if any(v is None for v in vals) else max(vals)
    ok = {m: v for m, v in worst.items() if v is not None}
    if not ok:
        return None, worst
    return min(ok, key=lambda m: (ok[m], m)), worst


def agree_placement(store, key: str, rank: int, world: int, mine: dict) -> tuple:
    """Every rank publishes its timings under ``key`` (c10d store) and computes
    :func:`choose_placement` over all of them - the same answer on every rank."""
    import json

    if store is None or world <= 1:
        return choose_placement([mine])
    store.set(f"{key}/{rank}", json.dumps({str(k): v for k, v in mine.items()}).encode())
    allt = [{int(k): v for k, v in json.loads(store.get(f"{key}/{r}").decode()).items()} for r in range(world)]
    return choose_placement(allt)


def chain_decision(same_all: bool, xgmi_ok_all: bool, oracle_ok_all: bool, have_rccl: bool) -> str:
    """What every rank does after the start-up check (all inputs already agreed across ranks):
    "keep" the production chain; "conservative" chain on the same plane (the production
    chain's bits differ from it); "rccl" (an xGMI wait timed out, or the xGMI reduction
    differs from the host oracle: the direct plane itself is not trusted); "fail" (that, with
    no RCCL plane to fall back to - a gloo control plane)."""
    if not xgmi_ok_all or not oracle_ok_all:
        return "rccl" if have_rccl else "fail"
    return "keep" if same_all else "conservative"


class FusedSimpleCNNEngine:
    def __init__(self, model, optimizer, data: DeviceMNIST, batch_size: int, world_size: int,
                 rank: int, comm=None, opts: EngineOptions | None = None, seed: int = 0):
        self.C = native.require()
        self.opts = dataclasses.replace(opts) if opts is not None else EngineOptions()
        self.model, self.opt, self.data = model, optimizer, data
        self.B = int(batch_size)
        pf1 = self.opts.dtype == "bf16" and bool(self.C.conv3x3_fwd_dz_fits(self.B, 28, 28, 1))
        if self.opts.pxt_fwd is None:
            self.opts.pxt_fwd = 1 if pf1 else 2
        if self.opts.dist_mode == 4 and pf1 and (world_size > 1 or self.opts.force_allreduce):
            self.opts.pxt_fwd = 1  # the step head runs the 256-thread forward in the all-reduce's blocks
        self.world_size, self.rank = world_size, rank
        self.fs = fs = flat_space(model)
        dev = fs.params.device
        if dev.type != "cuda":
            raise RuntimeError("the fused engine runs on a HIP device")
        names = {"w1": "net.0.weight", "b1": "net.0.bias", "w2": "net.2.weight",
                 "b2": "net.2.bias", "wfc": "fl.weight", "bfc": "fl.bias"}
        # any DDP bucket plan: each bucket's all-reduce starts as soon as its gradients are
        # final (fc-only buckets right after fc_bwd, overlapping the conv backward)
        from ..parallel.bucket_model import XgmiCost, engine_plan

        pw = self.opts.plan_world or world_size
        # the cost model's constants: a fit measured by this job before the engine was built
        # (bench.py at N > 1: comm_calibration.calibrate), else a stored fit for this world
        # size, else the defaults (XgmiCost.source records which)
        if self.opts.cost_fit is not None:
            self.cost = XgmiCost.from_fit(pw, self.opts.cost_fit,
                                          source=f"fit:{self.opts.cost_fit.get('topology', 'job')}")
        else:
            self.cost = XgmiCost.calibrated(pw)
        if self.opts.bucket_plan == "model":
            self.buckets, self.pred_comm_us = engine_plan(fs, pw, self.cost)
        elif self.opts.bucket_plan == "torch":
            self.buckets, self.pred_comm_us = bucket_plan(fs, self.opts.bucket_cap_mb, self.opts.first_bucket_mb), None
        else:
            raise ValueError(f"bucket_plan must be model|torch, got {self.opts.bucket_plan!r}")
        ranges = bucket_ranges(fs, self.buckets)
        offs = {k: fs.offsets[v] for k, v in names.items()}
        offs["buckets"] = [(int(o), int(n)) for o, n in ranges]
        self.sampler = ShardedSampler(len(data), world_size, rank, shuffle=True, seed=seed)
        n_rank = len(self.sampler)
        B, HW = self.B, 28 * 28
        if self.opts.dtype not in ("bf16", "fp32"):
            raise ValueError(f"engine dtype must be bf16 or fp32, got {self.opts.dtype!r}")
        f32 = self.opts.dtype == "fp32"
        self.store_a1 = self.opts.store_a1 if self.opts.store_a1 is not None else (0 if f32 else 1)
        if f32 and (self.opts.fuse_level < 1 or self.store_a1 != 0):
            raise ValueError("the fp32 engine runs the level-1 or level-3 chain (fuse_level >= 1, store_a1 0)")
        R = self.wgrad_rows = self.opts.wgrad_rows or wgrad_rows(28, B, torch.float32 if f32 else BF16)
        g = self.opt.param_groups[0]
        if g["momentum"] != 0 and self.opt.momentum_buffer is None:
            self.opt.momentum_buffer = torch.zeros_like(fs.params)
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
        self.steps_per_epoch = math.ceil(n_rank / B)
        if f32:  # fp32 activations + the conv2 weight's fp32 [tap][ci][co] copy; no bf16 buffers
            act = dict(a2=e(B * HW * 64), dz2=e(B * HW * 64), w2t_f32=e(64 * 9 * 32),
                       wfc_frag32=e(10 * HW * 64))
        else:
            act = dict(w2_bf16=e(64 * 9 * 32, dt=BF16), w2t_bf16=e(64 * 9 * 32, dt=BF16),
                       wfc_bf16=e(10 * HW * 64, dt=BF16), wfc_frag=e(10 * HW * 64, dt=BF16),
                       a1=e(B * HW * 32, dt=BF16), a2=e(B * HW * 64, dt=BF16),
                       dz2=e(B * HW * 64, dt=BF16), dz1=e(B * HW * 32, dt=BF16))
        self.t = dict(
            params=fs.params, grads=fs.grads,
            momentum=self.opt.momentum_buffer if self.opt.momentum_buffer is not None else e(1),
            **act,
            fc_part=e(2 * self.C.conv3x3_dgrad_blocks(B, 28, 28, self.opts.pxt_fwd) * 10),  # [blk][2][10]
            dlogits=e(B * 10), loss_rows=e(B),
            loss_hist=torch.zeros(self.steps_per_epoch + 1, device=dev),
            w2slab=e(self.C.conv3x3_wgrad_blocks(B, 28, R) * (64 * 9 * 32 + 64)),
            w1slab=e(self.C.conv3x3_dgrad_blocks(B, 28, 28, self.opts.pxt_dgrad) * 320),
            step_ctr=torch.zeros(1, dtype=torch.int32, device=dev),
            xb=torch.empty(B * HW, dtype=torch.uint8, device=dev),   # the step's batch (compact)
            yb=torch.empty(B, dtype=torch.int32, device=dev),
            images=(torch.empty(n_rank * HW, dtype=torch.uint8, device=dev) if self.opts.epoch_order
                    else data.images_u8.view(-1)),
            labels=(torch.empty(n_rank, dtype=torch.int32, device=dev) if self.opts.epoch_order
                    else data.labels_i32),
            idx=torch.zeros(n_rank, dtype=torch.int32, device=dev),
        )
        # in-launch hand-offs (fused slab reduction), zeroed by each step's forward, and their
        # wait-timeout word
        # (level 3: [256] the fc side kernel's last-block counter, [288, 288 + 2 * 64) dist_mode
        # 4's two bucket-done counters - runtime.h L3_HEAD_OFF; the level-3 forward's partial-logit
        # granules and their generation word are the native engine's own allocations)
        nfl = 256 + 32 + 64 * 2  # (counters 64 ints apart: FWD_DZ_CNT_STRIDE)
        self.t["sync_flags"] = torch.zeros(nfl, dtype=torch.int32, device=dev)
        # (the engine replaces it by a coherent host word: eng.sync_error)
        self.t["sync_err"] = torch.zeros(1, dtype=torch.int32, device=dev)
        cfg = dict(max_batch=B, H=28, W=28, C1=32, C2=64, NO=10, pxt_fwd=self.opts.pxt_fwd,
                   pxt_dgrad=self.opts.pxt_dgrad, wgrad_rows=R, world=world_size, rank=rank,
                   lr=float(g["lr"]), momentum=float(g["momentum"]),
                   dampening=float(g["dampening"]), weight_decay=float(g["weight_decay"]),
                   nesterov=bool(g["nesterov"]), maximize=bool(g["maximize"]),
                   force_allreduce=bool(self.opts.force_allreduce),
                   fuse_level=self._fuse_level_ok(world_size), fuse_opt=bool(self.opts.fuse_opt),
                   store_a1=int(self.store_a1), f32=f32, fuse_reduce=self._fuse_reduce_ok(world_size),
                   epoch_order=bool(self.opts.epoch_order), wgrad_split=int(self.opts.wgrad_split),
                   l3_fc_role=int(self.opts.l3_fc_role), dist_mode=int(self.opts.dist_mode))
        self.dtype = "fp32" if f32 else "bf16"
        use_comm = world_size > 1 or self.opts.force_allreduce
        self.xgmi = None
        self.xgmi_plan = None
        self.allreduce_us = None
        xch = list(range(len(ranges)))
        if use_comm and self.opts.comm in ("auto", "tune", "xgmi", "xgmi1", "xgmi2"):
            from ..parallel.xgmi import channel_plan, create_xgmi, pick_data_plane

            # small buckets also get a one-shot channel (one cross-GPU barrier instead of two)
            lim = self.cost.oneshot_cap_elems()
            oneshot = tuple(b for b, (_, n) in enumerate(ranges) if n <= lim)
            from ..parallel.xgmi import ENGINE_GRID_CAP

            cap = int(self.opts.xar_blocks) if self.opts.dist_mode == 2 else ENGINE_GRID_CAP
            self.xgmi = create_xgmi(fs.grads, ranges, rank, world_size, oneshot=oneshot, grid_cap=cap)
            if self.xgmi is not None and self.opts.comm in ("xgmi1", "xgmi2"):
                plan = "xgmi1" if self.opts.comm == "xgmi1" else "xgmi"  # forced (tests, sweeps)
            elif self.xgmi is not None and self.opts.comm in ("auto", "xgmi"):
                # deterministic: the plane depends only on the self-test outcome and the bucket
                # sizes, never on timing noise, so an uninterrupted run and a resumed run
                # reduce in the same order (BASELINE config 4).  Both xGMI plans sum in fixed
                # rank order 0..N-1, so they are bitwise interchangeable; RCCL is not.
                plan = "xgmi1" if oneshot else "xgmi"
            elif self.xgmi is not None:
                # "tune": measure one step's bucket all-reduces under each plan on this node
                # and keep the fastest (rank 0 decides for everyone); RCCL competes
                from ..parallel.xgmi import rccl_candidate_comms

                variants = rccl_candidate_comms(rank, world_size) if comm is not None else {}
                plan, self.allreduce_us, chosen = pick_data_plane(
                    self.xgmi, comm, fs.grads, ranges, rank, oneshot=oneshot, rccl_variants=variants)
                if plan.startswith("rccl"):
                    comm = chosen  # the tuned communicator (algorithm / protocol) becomes the plane
                # the candidates that lost are destroyed now (ncclCommDestroy, local), not kept
                # with their buffers and channels for the rest of the run
                variants = {k: c for k, c in variants.items() if c is comm}
                del variants
            if self.xgmi is not None:
                self.xgmi_plan = plan
                if plan.startswith("rccl"):
                    self.xgmi = None
                else:
                    cp = channel_plan(len(ranges), oneshot)
                    xch = [cp[(b, plan == "xgmi1" and b in oneshot)] for b in range(len(ranges))]
        if use_comm and self.xgmi is None and comm is None:
            raise RuntimeError("world size > 1 needs an RCCL communicator or the xGMI path")
        self.comm_kind = ((self.xgmi_plan or "xgmi") if self.xgmi is not None
                          else ((self.xgmi_plan if (self.xgmi_plan or "").startswith("rccl") else "rccl")
                                if use_comm else "none"))
        self.ranges, self.xch, self.comm = ranges, xch, (comm if use_comm else None)
        self.cfg, self.offs = cfg, offs
        self.chain_check = None  # verify_chain's outcome (dict), when it ran
        self.eng = self.C.SimpleCNNEngine(cfg, self.t, offs, comm if use_comm else None)
        if self.xgmi is not None:
            self.eng.set_xgmi(self.xgmi, xch)
        if self.opt.momentum_buffer is not None and self.opt.steps > 0:
            self.eng.set_momentum_started(True)
        self.stream = torch.cuda.ExternalStream(self.eng.stream, device=dev)
        # kernels per step of the chain that actually runs (engine.cpp / EngineConfig)
        self.level3 = bool(self.eng.level3_active(B))
        self._captured = 0
        self.steps_done = 0
        self._need_barrier = world_size > 1
        self._evaluators = {}  # {pxt: FusedEvaluator} (the inference kernel's scratch)

    # ------------------------------------------------------------------ start-up chain check
    def conservative_cfg(self) -> dict | None:
        """The conservative chain's config (level 1, separate grad_reduce kernel, same data
        plane), or None when the production chain already is that."""
        ref = dict(self.cfg, fuse_level=min(int(self.cfg["fuse_level"]), 1), fuse_reduce=0)
        return None if ref == self.cfg else ref

    def verify_chain(self, nsteps: int = 2, store=None, _corrupt_rank: int | None = None,
                     _corrupt_oracle_rank: int | None = None) -> bool:
        """VERDICT r3 #3a: before training commits to the production chain (level 3 + the
        fused slab reduction + the chosen data plane), run ``nsteps`` eager steps on it, then
        the same steps from the same snapshot on the conservative chain (level 1, separate
        grad_reduce, same plane), and compare parameters, momentum and losses bitwise.

        On the xGMI plane both chains share the all-reduce code, so step 1 is
        also checked against an oracle that does not use it: a comm-free engine computes this
        rank's local gradient from the same snapshot, every rank's local gradient is gathered
        over the process group and summed in rank order on the host (:func:`gather_rank_sum`),
        and the production chain's reduced gradient must equal it bit for bit on every bucket.

        Every rank publishes its verdicts through the store (:func:`agree`) and acts on the
        agreed ones (:func:`chain_decision`): a mismatch with the conservative chain -> every
        rank takes the conservative chain; an xGMI wait timeout or an oracle mismatch -> every
        rank takes RCCL (without an RCCL plane: a RuntimeError).  The snapshot (parameters,
        momentum, step counter, loss history, momentum state) is restored afterwards, so
        training starts exactly where it would have.  Collective at world size > 1.  Returns
        True when the production chain was kept."""
        ref_cfg = self.conservative_cfg()
        if ref_cfg is None and self.xgmi is None:
            self.chain_check = {"ran": False, "reason": "production chain is the conservative one"}
            return True
        if ref_cfg is None:  # (the oracle still runs; the "conservative" chain is this one)
            ref_cfg = dict(self.cfg)
        import torch.distributed as dist

        if store is None and dist.is_initialized() and self.world_size > 1:
            store = dist.distributed_c10d._get_default_store()
        t = self.t
        keys = ("params", "momentum", "step_ctr", "loss_hist")
        self.synchronize()
        torch.cuda.synchronize()
        snap = {k: t[k].clone() for k in keys}
        started = self.opt.momentum_buffer is not None and self.opt.steps > 0
        B = self.B

        def restore(e):
            # the copies (and start_epoch's index / epoch-order copies before them) are queued
            # on the production engine's stream, but engine e runs on its own: drain the device
            # before e derives its shadows and steps, or e could read the production run's
            # parameters / step counter
            with torch.cuda.stream(self.stream):
                for k in keys:
                    t[k].copy_(snap[k])
            torch.cuda.synchronize()
            e.set_momentum_started(started)
            e.refresh_shadows()
            torch.cuda.synchronize()

        # dist_mode 4: the step head (a pair launch carrying the next forward) exists only in a
        # captured graph, so the production chain runs its steps as one (momentum-init step
        # eager) - with at least one step head in it
        head = bool(self.eng.overlap_active())
        if head:
            nsteps = max(nsteps, 3)

        def run(e, graph=False):
            """nsteps on engine e from the snapshot -> (params, momentum, losses) or an error."""
            self.start_epoch(0)
            restore(e)
            try:
                if graph:
                    left = nsteps
                    if self.opt.momentum_buffer is not None and not started:
                        e.step(B, B)  # (the momentum buffer's initialising step is eager)
                        left -= 1
                    e.capture(left)
                    e.replay()
                else:
                    for _ in range(nsteps):
                        e.step(B, B)
                e.synchronize()
            except RuntimeError as ex:  # an in-launch wait timed out
                return None, f"in-launch wait: {ex}"
            if self.xgmi is not None and self.xgmi.error_flags():
                from ..parallel.xgmi import describe_xgmi_error

                return None, "xgmi: " + describe_xgmi_error(self.xgmi.error_flags())
            torch.cuda.synchronize()
            return [t[k].clone() for k in ("params", "momentum")] + [t["loss_hist"][:nsteps].clone()], None

        ref = self.C.SimpleCNNEngine(ref_cfg, t, self.offs, self.comm)
        if self.xgmi is not None:
            ref.set_xgmi(self.xgmi, self.xch)
        got, err_p = run(self.eng, graph=head)
        heads_checked = int(self.eng.graph_heads) if head else 0
        if head:
            self.eng.destroy_graph()
            self._captured = 0
        if got is not None and _corrupt_rank == self.rank:  # test hook: a one-ulp disagreement
            got[0][0] = torch.nextafter(got[0][0], torch.tensor(float("inf"), device=got[0].device))
        pair_ran = bool(self.eng.last_pair)
        want, err_r = run(ref)
        same = got is not None and want is not None and all(torch.equal(a, b) for a, b in zip(got, want))
        xgmi_bad = (err_p or "").startswith("xgmi") or (err_r or "").startswith("xgmi")
        # ---- the independent oracle (xGMI plane: its sum order is fixed, so bits must match)
        oracle = {"ran": False}
        oracle_ok = True
        if self.xgmi is not None and not xgmi_bad:
            oracle_ok, oracle = self._reduce_oracle(restore, _corrupt_oracle_rank)
            xgmi_bad = xgmi_bad or oracle.get("xgmi_error") is not None
        key = f"ddp_amd/chain/{FusedSimpleCNNEngine._chain_gen}"
        FusedSimpleCNNEngine._chain_gen += 1
        ok_all = agree(store, key + "/same", self.rank, self.world_size, same)
        x_ok_all = agree(store, key + "/xgmi", self.rank, self.world_size, not xgmi_bad)
        o_ok_all = agree(store, key + "/oracle", self.rank, self.world_size, oracle_ok)
        action = chain_decision(ok_all, x_ok_all, o_ok_all, self.comm is not None)
        chosen = self.eng
        if action == "fail":
            raise RuntimeError("start-up chain check: the xGMI data plane "
                               f"{'timed out' if not x_ok_all else 'disagrees with the host oracle'} "
                               f"({oracle}) and there is no RCCL plane")
        if action == "rccl":
            self.xgmi, self.xgmi_plan, self.comm_kind = None, "rccl", "rccl"
            chosen = self.C.SimpleCNNEngine(ref_cfg, t, self.offs, self.comm)
            why = "xGMI wait timed out" if not x_ok_all else "xGMI reduction differs from the host oracle"
            self._log_downgrade(f"start-up chain check: {why} -> conservative chain over RCCL")
        elif action == "conservative":
            chosen = ref
            self._log_downgrade("start-up chain check: production chain differs from the conservative one "
                                f"(here: {'same' if same else err_p or err_r or 'bits differ'}) -> conservative chain")
        if chosen is not self.eng:
            self.eng = chosen
            self.cfg = ref_cfg
            self.stream = torch.cuda.ExternalStream(self.eng.stream, device=self.fs.params.device)
            self.level3 = bool(self.eng.level3_active(B))
            self._captured = 0
        self.start_epoch(0)
        restore(self.eng)
        torch.cuda.synchronize()
        self.chain_check = {"ran": True, "steps": nsteps, "identical_here": same, "identical_all": ok_all,
                            "xgmi_ok_all": x_ok_all, "oracle_ok_all": o_ok_all, "oracle": oracle,
                            "pair": pair_ran, "step_heads_checked": heads_checked,
                            "kept_production": action == "keep",
                            "error": err_p or err_r}
        return self.chain_check["kept_production"]

    _chain_gen = 0

    def _reduce_oracle(self, restore, corrupt_rank=None):
        """Step 1 of the production chain vs the host oracle (see :meth:`verify_chain`):
        (ok_here, info).  ``restore(e)`` resets the snapshot for engine ``e``.  Collective."""
        t, B = self.t, self.B
        # this rank's local gradient, prescaled by 1 / world exactly as the production
        # producers write it: the same chain without any data plane and without the fused
        # optimizer (the gradient buffer keeps the gradient; its SGD pass is undone by restore)
        loc_cfg = dict(self.cfg, force_allreduce=False, fuse_opt=False)
        loc = self.C.SimpleCNNEngine(loc_cfg, t, self.offs, None)
        self.start_epoch(0)
        restore(loc)
        loc.step(B, B)
        loc.synchronize()
        torch.cuda.synchronize()
        local = t["grads"].detach().clone()
        self.start_epoch(0)
        restore(self.eng)
        self.eng.step(B, B)
        info = {"ran": True, "buckets": len(self.ranges)}
        try:
            self.eng.synchronize()
        except RuntimeError as ex:
            info["xgmi_error"] = f"in-launch wait: {ex}"
        if self.xgmi.error_flags():
            from ..parallel.xgmi import describe_xgmi_error

            info["xgmi_error"] = describe_xgmi_error(self.xgmi.error_flags())
        torch.cuda.synchronize()
        reduced = t["grads"].detach().clone()
        if corrupt_rank == self.rank:  # test hook: one ulp off in this rank's reduced bucket
            off = int(self.ranges[0][0])
            reduced[off] = torch.nextafter(reduced[off], torch.tensor(float("inf"), device=reduced.device))
        want = gather_rank_sum(local, self.world_size)
        bad = oracle_mismatches(reduced, want, self.ranges)
        info["mismatches"] = bad
        return bad == 0 and "xgmi_error" not in info, info

    # ------------------------------------------------------------------ helpers
    def _device_shared(self, world_size: int) -> bool:
        """Whether any GPU of the job runs more than one rank (same-GPU rehearsals).

        Decided from every rank's PCI bus id through the c10d store, so it is right when
        each rank sees only its own device (HIP_VISIBLE_DEVICES isolation) and across nodes
        (ADVICE r3); without a process group, by the visible device count.  Cached."""
        if getattr(self, "_shared", None) is not None:
            return self._shared
        shared = False
        if world_size > 1:
            import torch.distributed as dist

            if dist.is_initialized():
                from ..parallel.xgmi import max_sharing

                store = dist.distributed_c10d._get_default_store()
                key = f"ddp_amd/engine_bus/{FusedSimpleCNNEngine._bus_gen}"
                FusedSimpleCNNEngine._bus_gen += 1
                dev = self.fs.params.device.index
                store.set(f"{key}/{self.rank}", self.C.pci_bus_id(dev).encode())
                shared = max_sharing(store.get(f"{key}/{r}").decode() for r in range(world_size)) > 1
            else:
                shared = torch.cuda.device_count() < world_size
        self._shared = shared
        return shared

    _bus_gen = 0

    def _fuse_level_ok(self, world_size: int) -> int:
        """Level 3's forward spins on the other blocks of its images, which must all be
        resident: ranks that share a device (same-GPU rehearsals) would split the GPU
        between two such forwards, so they run the level-1 chain instead (logged)."""
        lvl = int(self.opts.fuse_level)
        # DDP_AMD_SHARED_GPU_L3=1 (multi-rank tests on one GPU, small batches): keep level 3 -
        # and with it the step head - when the ranks' grids together fit the GPU; a wait that
        # cannot complete is bounded and raises (the start-up check then downgrades)
        if lvl >= 3 and self._device_shared(world_size) and os.environ.get("DDP_AMD_SHARED_GPU_L3") != "1":
            self._log_downgrade("fuse level 3 -> 1 (a GPU is shared by several ranks)")
            return 1
        return lvl

    def _fuse_reduce_ok(self, world_size: int) -> int:
        """The fused reduction's waiting blocks are sized against ONE launch's share of the
        GPU; ranks that share a device (same-GPU rehearsals) each hold waiting blocks at
        once, so they keep the separate grad_reduce kernel (logged)."""
        fr = self.opts.fuse_reduce
        if fr is None:  # (the in-launch all-reduce, dist_mode 2, needs the fused reduction)
            fr = 0 if self.opts.dtype == "fp32" and self.opts.dist_mode != 2 else 1
        if not fr:
            return 0
        if self._device_shared(world_size):
            self._log_downgrade("fused slab reduction off (a GPU is shared by several ranks)")
            return 0
        return int(fr)

    def _log_downgrade(self, what: str):
        self.downgrades = getattr(self, "downgrades", []) + [what]
        if self.rank == 0:
            import sys

            print(f"[ddp_amd] engine: {what}", file=sys.stderr)

    def sync_from_torch(self):
        """Order the engine stream after work queued on torch's current stream."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.stream.wait_event(ev)

    def refresh(self):
        """Re-derive bf16 shadows from the fp32 master weights (after init/load)."""
        self.sync_from_torch()
        self.eng.refresh_shadows()

    def synchronize(self):
        self.eng.synchronize()
        self._check_xgmi("step")

    def _check_xgmi(self, where: str):
        if self.xgmi is not None:
            code = self.xgmi.error_flags()
            if code:
                from ..parallel.xgmi import describe_xgmi_error

                raise RuntimeError(f"xGMI all-reduce ({where}) on rank {self.rank}: "
                                   f"{describe_xgmi_error(code)}; results invalid")

    def _start_barrier(self):
        """Before the first step of a multi-rank run (after start-up and after a resume): a
        host barrier, so rank skew from construction / checkpoint loading is not spent inside
        the first all-reduce's device-side barrier spin."""
        if self._need_barrier:
            self._need_barrier = False
            import torch.distributed as dist

            if dist.is_initialized() and dist.get_world_size() > 1:
                torch.cuda.current_stream().synchronize()
                self.stream.synchronize()
                dist.barrier()

    def _ensure_graph(self):
        k = self.opts.graph_steps
        if self.opts.use_graph and self._captured != k:
            self.eng.capture(k)
            self._captured = k

    def measure_bucket_allreduce(self, iters: int = 20) -> list | None:
        """Device time (us) of each bucket's all-reduce on the engine's data plane, in
        isolation (collective: every rank calls it).  Clobbers the gradient buffer - the
        step rewrites every bucket, so call it between steps only."""
        if self.comm_kind == "none":
            return None
        self.synchronize()
        out = []
        for b, (off, n) in enumerate(self.ranges):
            if self.xgmi is not None:
                fn = lambda ch=self.xch[b]: self.xgmi.all_reduce(ch)  # noqa: E731
            else:
                view = self.fs.grads[off:off + n]
                fn = lambda v=view: self.comm.all_reduce(v)  # noqa: E731
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out.append(round(e0.elapsed_time(e1) * 1000.0 / iters, 2))
        self._check_xgmi("bucket timing")
        return out

    # ------------------------------------------------------------------ evaluation
    def eval_operands(self) -> dict:
        """What the training forward reads - conv1's parameters, the conv2 OHWI weight (bf16
        shadow / fp32 master), b2, the fc weight in the FCFRAG order and the fc bias - all kept
        current by the fused SGD, so an evaluation needs no refresh."""
        fs, t = self.fs, self.t
        v = lambda n: fs.view(fs.params, n).detach().reshape(-1)  # noqa: E731
        f32 = self.dtype == "fp32"
        return dict(w1=v("net.0.weight"), b1=v("net.0.bias"),
                    w2=v("net.2.weight") if f32 else t["w2_bf16"], b2=v("net.2.bias"),
                    wfc_frag=t["wfc_frag32"] if f32 else t["wfc_frag"], bfc=v("fl.bias"))

    def evaluate(self, data: DeviceMNIST, batch_size: int = 1000, indices=None, pxt: int = 2,
                 want_logits: bool = False):
        """Accuracy and loss of the CURRENT parameters over rows ``indices`` (default: all) of
        ``data``: one fused inference launch per batch (ragged last batch included), eagerly on
        the engine's stream - behind whatever training work is queued - with scratch of its
        own.  Returns an :class:`~ddp_amd.engine.evaluation.EvalResult` (``correct``, ``count``,
        ``loss_sum`` and the per-image ``pred`` / ``loss`` tensors).  ``pxt`` = the engine's
        ``opts.pxt_fwd`` reproduces the training forward's summation order bit for bit."""
        from .evaluation import FusedEvaluator

        ev = self._evaluators.get(pxt)
        if ev is None:
            ev = self._evaluators[pxt] = FusedEvaluator(self.fs.params.device, self.dtype, pxt)
        self.sync_from_torch()  # (the split / index tensors may have been made on torch's stream)
        with torch.cuda.stream(self.stream):
            res = ev.run(data, self.eval_operands(), batch_size, indices, want_logits)
        for out in (res.pred, res.loss, res.logits, res.correct_rows):
            if out is not None:
                out.record_stream(torch.cuda.current_stream())
        return res

    # ------------------------------------------------------------------ epoch
    def start_epoch(self, epoch: int):
        self.sampler.set_epoch(epoch)
        # once per epoch, 240 KB: a synchronous pageable copy ordered on the engine stream
        # (no pinned block is ever tied to the engine's stream)
        idx = self.sampler.indices().to(torch.int32)
        with torch.cuda.stream(self.stream):
            self.t["idx"].copy_(idx)
            if self.opts.epoch_order:  # the rank's samples in this epoch's order
                n, HW = self.t["idx"].numel(), 28 * 28
                torch.index_select(self.data.images_u8.view(-1, HW), 0, self.t["idx"],
                                   out=self.t["images"].view(n, HW))
                torch.index_select(self.data.labels_i32, 0, self.t["idx"], out=self.t["labels"])
            self.t["step_ctr"].zero_()
            self.t["loss_hist"].zero_()

    def run_epoch(self, epoch: int, on_loss=None, log_every: int = 100, max_steps: int | None = None):
        """Train one epoch; ``on_loss(batch_idx, loss)`` is called for batch_idx % log_every == 0.

        ``max_steps`` truncates the epoch (smoke runs, fault injection)."""
        self._start_barrier()
        self.sync_from_torch()
        self.start_epoch(epoch)
        n = len(self.sampler)
        B = self.B
        nfull, rem = divmod(n, B)
        if max_steps is not None and max_steps < nfull + (1 if rem else 0):
            nfull, rem = max_steps, 0
        done = 0
        pending = []  # (first_batch, last_batch_exclusive, event)
        if self.opt.momentum_buffer is not None and not self.opt.steps and nfull > 0:
            self.eng.step(B, B)  # momentum buffer initialisation step (torch semantics)
            done, self.opt.steps = 1, 1
            pending.append((0, 1, self._event()))
        k = self.opts.graph_steps
        if self.opts.use_graph and nfull - done >= k:
            self._ensure_graph()
        while done < nfull:
            if self.opts.use_graph and self._captured == k and nfull - done >= k:
                self.eng.replay()
                pending.append((done, done + k, self._event()))
                done += k
            else:
                self.eng.step(B, B)
                pending.append((done, done + 1, self._event()))
                done += 1
            self._drain(pending, on_loss, log_every, keep=1)
        if rem:
            self.eng.step(rem, B)
            pending.append((done, done + 1, self._event()))
            done += 1
        self._drain(pending, on_loss, log_every, keep=0)
        self.steps_done += done
        self.opt.steps += done
        return done

    def run_steps(self, nsteps: int, head: int = 0):
        """Benchmark helper: ``nsteps`` full-batch steps (graph replays when possible).

        Walks epoch 0's index list and wraps to its start when a replay would run
        past the last full batch (the device step counter is reset on the stream).
        ``head``: launch the first ``head`` steps eagerly (two kernel launches each, the
        GPU starts on the first at once) so the host-side graph launch of the rest
        overlaps them instead of delaying the first kernel.
        """
        self._start_barrier()
        if not self._bench_started:
            self.sync_from_torch()
            self.start_epoch(0)
            self._bench_started = True
        k = self.opts.graph_steps
        n_full = len(self.sampler) // self.B
        done = init = 0
        if nsteps > 0 and self.opt.momentum_buffer is not None and not self.opt.steps:
            self._wrap_if_needed(1, n_full)
            self.eng.step(self.B, self.B)  # momentum buffer initialisation step (eager)
            done = init = 1
            self.opt.steps = 1
        while done < nsteps:
            if self.opts.use_graph and done >= head and nsteps - done >= k and k <= n_full:
                self._ensure_graph()
                self._wrap_if_needed(k, n_full)
                self.eng.replay()
                done += k
            else:
                self._wrap_if_needed(1, n_full)
                self.eng.step(self.B, self.B)
                done += 1
        self.steps_done += done
        self.opt.steps += done - init
        return done

    _bench_started = False
    _bench_pos = 0

    def _wrap_if_needed(self, k, n_full):
        if self._bench_pos + k > n_full:
            with torch.cuda.stream(self.stream):
                self.t["step_ctr"].zero_()
            self._bench_pos = 0
        self._bench_pos += k

    def _event(self):
        ev = torch.cuda.Event()
        ev.record(self.stream)
        return ev

    def _drain(self, pending, on_loss, log_every, keep):
        while len(pending) > keep:
            first, last, ev = pending.pop(0)
            want = [b for b in range(first, last) if b % log_every == 0]
            if not want or on_loss is None:
                continue
            ev.synchronize()
            vals = self.t["loss_hist"][want].tolist()
            for b, v in zip(want, vals):
                on_loss(b, v)
