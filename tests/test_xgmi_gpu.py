"""Direct xGMI all-reduce (csrc/kernels/allreduce.hip) and the engine's multi-rank path.

RCCL refuses two ranks on one GPU ("Duplicate GPU detected"), but the xGMI path only needs
IPC mappings, which also work between processes sharing a device.  So these tests run 2
(some also 3) ranks on cuda:0 of the single-GPU test box (gloo process group for bootstrap
only) and exercise the exact kernel, protocol and engine code that runs across 8 GPUs.  Not
more than 3: the kernel's barriers spin until the peers' blocks arrive, which on ONE GPU needs
every rank's kernel resident at once - the GPU runs two processes' queues side by side,
but with more it time-slices them and a barrier can wait seconds (measured with
scripts/xgmi_probe.py: correct sums, 17-40 s stalls).  With one GPU per rank (the real
deployment) every rank's kernel has its own device.

World sizes above 3 and the sweep over bucket lengths, offsets, grids and fused-SGD options
live in tests/test_xgmi_loopback_gpu.py: N = 1..8 virtual ranks of the same kernel body in one
launch of one process.  What that cannot show - real IPC mappings, skew between the ranks'
launches across calls, the pair kernel's completion count - is covered here.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _allreduce_worker(rank, world, port, q):
    try:
        _init(rank, world, port)
        from ddp_amd.parallel import create_xgmi

        # odd lengths and offsets: 16-byte quads with partial tails, unaligned bases; the
        # third bucket (10 elements at an odd offset, like fl.bias) leaves rank 1 a 2-element slice
        n_total = 501_770 + 18_816 + 1 + 10 + 64
        buckets = [(0, 501_770), (501_770, 18_816), (520_587, 10)]
        grads = torch.zeros(n_total, device="cuda")
        x = create_xgmi(grads, buckets, rank, world, oneshot=(1,))  # channel 3: one-shot bucket 1
        assert x is not None, "self-test failed"
        assert x.channels == 4 and x.oneshot(3) and not x.oneshot(1)
        # two ranks on one GPU: every spinning grid leaves room for the other's kernels
        assert max(x.blocks(c) for c in range(4)) <= 32
        for it in range(4):
            g = torch.Generator().manual_seed(1000 * it + rank)
            mine = torch.randn(n_total, generator=g)
            grads.copy_(mine.cuda())
            torch.cuda.synchronize()
            x.all_reduce(0)
            x.all_reduce(1, scale=0.5)
            x.all_reduce(2)
            torch.cuda.synchronize()
            assert x.error_flags() == 0
            allin = [None] * world
            dist.all_gather_object(allin, mine)
            want = allin[0].clone()
            for r in range(1, world):
                want += allin[r]  # the kernel's fixed rank order, fp32
            got = grads.cpu()
            b0, b1 = buckets[:2]
            assert torch.equal(got[:b0[1]], want[:b0[1]]), f"bucket 0 it {it}"
            s1 = slice(b1[0], b1[0] + b1[1])
            assert torch.equal(got[s1], want[s1] * 0.5), f"bucket 1 it {it}"
            b2 = buckets[2]
            assert torch.equal(got[b2[0]:b2[0] + b2[1]], want[b2[0]:b2[0] + b2[1]]), f"bucket 2 it {it}"
            assert got[b1[0] + b1[1]] == mine[b1[0] + b1[1]], "gap between buckets touched"
            assert torch.equal(got[b2[0] + b2[1]:], mine[b2[0] + b2[1]:]), "outside the buckets"
            # the one-shot channel over bucket 1: same bits as the two-shot one
            grads.copy_(mine.cuda())
            torch.cuda.synchronize()
            x.all_reduce(3, scale=0.5)
            torch.cuda.synchronize()
            assert x.error_flags() == 0
            got1 = grads.cpu()
            assert torch.equal(got1[s1], want[s1] * 0.5), f"one-shot bucket 1 it {it}"
            assert torch.equal(got1[:b0[1]], mine[:b0[1]]), "one-shot touched bucket 0"
            # DDP's averaging: every rank's values times 1/3 BEFORE the
            # rank-order sum (publish pass of the two-shot kernel / the one-shot publish)
            s3 = torch.tensor(1.0 / 3.0, dtype=torch.float32)
            want3 = allin[0] * s3
            for r in range(1, world):
                want3 = want3 + allin[r] * s3
            for ch, sl in ((0, slice(0, b0[1])), (3, s1)):
                grads.copy_(mine.cuda())
                torch.cuda.synchronize()
                x.all_reduce(ch, publish=True, prescale=1.0 / 3.0)
                torch.cuda.synchronize()
                assert x.error_flags() == 0
                assert torch.equal(grads.cpu()[sl], want3[sl]), f"prescaled channel {ch} it {it}"
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))


def _engine_worker(rank, world, port, q, comm="xgmi2"):
    try:
        _init(rank, world, port)
        from ddp_amd.data import DeviceMNIST, synthetic_mnist
        from ddp_amd.engine import EngineOptions, FusedSimpleCNNEngine
        from ddp_amd.models import SimpleCNN
        from ddp_amd.models.layers import flat_space
        from ddp_amd.ops import FusedSGD

        torch.manual_seed(0)
        model = SimpleCNN().cuda()
        fs = flat_space(model)
        opt = FusedSGD(model, lr=0.05, momentum=0.9)
        imgs, labels = synthetic_mnist(4096)
        eng = FusedSimpleCNNEngine(model, opt, DeviceMNIST(imgs, labels, torch.device("cuda", 0)),
                                   16, world, rank, None, EngineOptions(graph_steps=5, comm=comm))
        assert eng.comm_kind == ("xgmi1" if comm == "xgmi1" else "xgmi"), eng.comm_kind
        eng.refresh()
        p0 = fs.params.detach().cpu().clone()
        eng.run_steps(1)
        eng.synchronize()
        p_one = fs.params.detach().cpu().clone()
        eng.run_steps(15)
        eng.synchronize()
        # the default multi-GPU chain's all-reduce launch (dist_mode 3: both buckets in one
        # xgmi_allreduce_pair launch) ran with a real second rank - on the level-1 chain that
        # ranks sharing a GPU run
        assert eng.eng.last_pair, "the dist_mode 3 pair launch did not run"
        p = fs.params.detach().cpu()
        allp = [None] * world
        dist.all_gather_object(allp, p)
        for r in range(world):
            assert torch.equal(allp[r], allp[0]), f"rank {r} params differ from rank 0"
        assert torch.isfinite(p).all()
        if rank == 0:
            # DDP semantics: 2 ranks x 16 (DistributedSampler shards of the same 32-image
            # window) == 1 rank x 32, up to summation order
            # (one step: longer runs drift apart through bf16 weight-shadow roundings)
            torch.manual_seed(0)
            m1 = SimpleCNN().cuda()
            f1 = flat_space(m1)
            assert torch.equal(f1.params.detach().cpu(), p0)
            o1 = FusedSGD(m1, lr=0.05, momentum=0.9)
            e1 = FusedSimpleCNNEngine(m1, o1, DeviceMNIST(imgs, labels, torch.device("cuda", 0)),
                                      32, 1, 0, None, EngineOptions(graph_steps=5))
            e1.refresh()
            e1.run_steps(1)
            e1.synchronize()
            d1 = f1.params.detach().cpu() - p0
            d2 = p_one - p0
            err = ((d2 - d1).norm() / d1.norm()).item()
            assert err < 1e-4, f"2-rank xGMI step vs 1-rank step: rel err of the update {err:.2e}"
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", float(p.double().sum())))  # plain float: no shared-memory tensor
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e), None))


def _module_grad_worker(rank, world, port, q):
    """Module-path DDP (native reducer, xGMI data plane): the all-reduced gradient is
    bitwise the rank-order sum of every rank's local gradient times 1/world."""
    try:
        _init(rank, world, port)
        from ddp_amd.models import SimpleCNN
        from ddp_amd.models.layers import flat_space
        from ddp_amd.ops import CrossEntropyLoss
        from ddp_amd.parallel import DistributedDataParallel

        dev = torch.device("cuda", 0)
        lossf = CrossEntropyLoss()
        g = torch.Generator().manual_seed(100 + rank)
        x = torch.randn(8, 1, 28, 28, generator=g).to(dev)
        y = torch.randint(0, 10, (8,), generator=g).to(dev)
        torch.manual_seed(0)
        twin = SimpleCNN(compute_dtype=torch.float32).to(dev)  # no DDP: the local gradient
        lossf(twin(x), y).backward()
        local = flat_space(twin).grads.detach().cpu().clone()
        torch.manual_seed(0)
        model = SimpleCNN(compute_dtype=torch.float32).to(dev)
        ddp = DistributedDataParallel(model, comm="xgmi", bucket_cap_mb=0.05, first_bucket_mb=0.05)
        assert ddp.comm_kind == "xgmi", ddp.comm_kind
        lossf(ddp(x), y).backward()
        torch.cuda.synchronize()
        got = flat_space(model).grads.detach().cpu()
        alll = [None] * world
        dist.all_gather_object(alll, local)
        s = torch.tensor(1.0 / world, dtype=torch.float32)
        want = alll[0] * s
        for r in range(1, world):
            want = want + alll[r] * s
        ok = torch.equal(got, want) and ddp._native.xgmi.error_flags() == 0
        msg = "ok" if ok else f"mismatch: max |diff| {(got - want).abs().max().item():.3e}, nb {len(ddp.buckets)}"
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, msg))
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, repr(e) + traceback.format_exc()[-600:]))


def _run(worker, world, port, *extra):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + extra) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    return res


@pytest.mark.parametrize("world", [2])
def test_xgmi_allreduce_exact(world):
    from ddp_amd.parallel import free_port

    res = _run(_allreduce_worker, world, free_port())
    assert all(r[1] == "ok" for r in res), res


@pytest.mark.parametrize("comm", ["xgmi2", "xgmi1"])
def test_engine_two_ranks_xgmi_identical_params(comm):
    """Both xGMI plans: two-shot for both buckets, and the one-shot kernel for the small
    conv bucket."""
    from ddp_amd.parallel import free_port

    res = _run(_engine_worker, 2, free_port(), comm)
    assert all(r[1] == "ok" for r in res), [r[:2] for r in res]


def _head_worker(rank, world, port, q):
    """The default multi-GPU chain (level 3 + dist_mode 4: step k's bucket all-reduces and step
    k + 1's forward in one launch) with a real second rank on the same GPU: B = 8 per rank so
    both ranks' grids fit the GPU together (DDP_AMD_SHARED_GPU_L3), the start-up check with the
    host oracle (every rank's local gradient gathered over gloo and summed in rank order),
    then graph replays with step heads; parameters bit-identical across ranks."""
    try:
        os.environ["DDP_AMD_SHARED_GPU_L3"] = "1"
        os.environ["DDP_AMD_XGMI_GRID_CAP"] = "16"  # (the channels' role blocks, per rank)
        _init(rank, world, port)
        from ddp_amd.data import DeviceMNIST, synthetic_mnist
        from ddp_amd.engine import EngineOptions, FusedSimpleCNNEngine
        from ddp_amd.models import SimpleCNN
        from ddp_amd.models.layers import flat_space
        from ddp_amd.ops import FusedSGD

        torch.manual_seed(0)
        model = SimpleCNN().cuda()
        fs = flat_space(model)
        opt = FusedSGD(model, lr=0.05, momentum=0.9)
        imgs, labels = synthetic_mnist(2048)
        eng = FusedSimpleCNNEngine(model, opt, DeviceMNIST(imgs, labels, torch.device("cuda", 0)),
                                   8, world, rank, None, EngineOptions(graph_steps=5, comm="xgmi1"))
        assert eng.level3 and eng.opts.dist_mode == 4, (eng.level3, eng.opts.dist_mode)
        eng.refresh()
        assert eng.eng.overlap_active()
        assert eng.verify_chain(), eng.chain_check
        ck = eng.chain_check
        assert ck["oracle"]["ran"] and ck["oracle"]["mismatches"] == 0 and ck["step_heads_checked"] >= 1, ck
        eng.run_steps(11)  # the momentum-init step eager, then two 5-step graphs with step heads
        eng.synchronize()
        assert eng.eng.sync_error == 0 and eng.eng.graph_heads == 4, eng.eng.graph_heads
        p = fs.params.detach().cpu()
        allp = [None] * world
        dist.all_gather_object(allp, p)
        for r in range(world):
            assert torch.equal(allp[r], allp[0]), f"rank {r} params differ from rank 0"
        assert torch.isfinite(p).all()
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, f"{e!r}\n{traceback.format_exc()}"))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_step_head_two_real_ranks(world):
    """VERDICT r5 missing #1 for the round-6 default chain: the step head with real peers
    (2 and 3 ranks on one GPU, B = 8 each)."""
    from ddp_amd.parallel import free_port

    res = _run(_head_worker, world, free_port())
    assert all(r[1] == "ok" for r in res), [r[:2] for r in res]


def _pair_worker(rank, world, port, q, ncalls):
    """The production dist_mode 3 launch (xgmi_allreduce_pair: the fc bucket two-shot and the
    conv bucket one-shot side by side, SGD + momentum fused into the all-gathers) with real
    peer ranks, against an oracle that does not use the xGMI code: every rank's bucket
    gathered over gloo and added in rank order on the host, then the plain SGD kernel."""
    try:
        _init(rank, world, port)
        from ddp_amd import native
        from ddp_amd.parallel import create_xgmi

        C = native.require()
        dev = torch.device("cuda", 0)
        n_fc, n_conv = 501_770, 18_816  # SimpleCNN's two buckets
        n = n_fc + n_conv
        grads = torch.zeros(n, device=dev)
        x = create_xgmi(grads, [(0, n_fc), (n_fc, n_conv)], rank, world, oneshot=(1,))
        assert x is not None, "self-test failed"
        assert x.oneshot(2) and not x.oneshot(1)
        params = torch.randn(n, generator=torch.Generator().manual_seed(7)).to(dev)  # same on every rank
        mom = torch.zeros_like(params)
        ref_p, ref_m = params.clone(), mom.clone()
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        lr, mu = 0.05, 0.9
        pairs_run = set()
        for it in range(ncalls):
            # mostly the production pairing (fc two-shot + conv one-shot); every third call both
            # two-shot - each channel sees both stage parities
            ch1 = 1 if it % 3 == 0 else 2
            pairs_run.add(ch1)
            g = torch.Generator().manual_seed(1000 * it + rank)
            mine = torch.randn(n, generator=g) * (1.0 / world)  # prescaled, as the producers write it
            grads.copy_(mine.to(dev))
            torch.cuda.synchronize()
            x.all_reduce_pair(0, ch1, params, mom, lr=lr, momentum=mu, first_step=it == 0, step_ctr=step)
            torch.cuda.synchronize()
            assert x.error_flags() == 0, x.error_flags()
            allin = [None] * world
            dist.all_gather_object(allin, mine)
            want = allin[0].clone()
            for r in range(1, world):
                want += allin[r]  # rank order 0..world-1, fp32
            got = grads.cpu()
            if not torch.equal(got, want):
                bad = (got != want).nonzero().flatten()
                raise AssertionError(f"call {it} (ch {ch1}): {bad.numel()} elements differ, first {bad[:4].tolist()}")
            C.sgd(ref_p, want.to(dev), ref_m, lr, mu, 0.0, 0.0, False, False, it == 0, True, [])
            torch.cuda.synchronize()
            assert torch.equal(params, ref_p) and torch.equal(mom, ref_m), f"call {it}: fused SGD differs"
        assert int(step.item()) == ncalls, int(step.item())
        assert pairs_run == {1, 2}
        allp = [None] * world
        dist.all_gather_object(allp, torch.cat([params.cpu(), mom.cpu()]))
        assert all(torch.equal(a, allp[0]) for a in allp), "replicas differ"
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, repr(e) + traceback.format_exc()[-800:]))


@pytest.mark.parametrize("world", [2, 3])
def test_pair_launch_multirank_oracle(world):
    """the default multi-GPU all-reduce launch with 2 and 3 real ranks on one
    GPU, 50 calls each (both stage parities of every channel), bitwise against the rank-order
    host sum and the SGD kernel, replicas identical, the step counter advanced once per call."""
    from ddp_amd.parallel import free_port

    res = _run(_pair_worker, world, free_port(), 50)
    assert all(r[1] == "ok" for r in res), res


def _calib_worker(rank, world, port, q, out):
    try:
        _init(rank, world, port)
        from ddp_amd.parallel import comm_calibration as cc

        fit = cc.calibrate(rank, world, torch.device("cuda", 0))
        topo = cc.topology(world, rank=rank)
        if rank == 0:
            cc.save(fit, world, topo, path=out)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", fit, topo))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e), None, None))


def test_comm_calibration_same_gpu(tmp_path):
    """the cost-model fit from timed sweeps of both bucket kernels (2 ranks on
    one GPU): every rank gets rank 0's constants, the fit is finite and explains the
    timings, and it is stored as a same-GPU record (not used for real xGMI plans)."""
    from ddp_amd.parallel import free_port
    from ddp_amd.parallel import comm_calibration as cc
    from ddp_amd.parallel.bucket_model import XgmiCost

    out = str(tmp_path / "cal.json")
    res = _run(_calib_worker, 2, free_port(), out)
    assert all(r[1] == "ok" for r in res), [r[:2] for r in res]
    fits = [r[2] for r in res]
    assert fits[0] == fits[1] and fits[0] is not None
    f = fits[0]
    assert f["n"] == 2 * len(cc.SWEEP_ELEMS) and all(v >= 0 for v in (f["launch_us"], f["barrier_us"]))
    assert f["rms_us"] < 0.25 * max(t for _, _, t in f["samples"])
    assert res[0][3] == "same-gpu"
    assert cc.load(out)["same-gpu/2"]["world"] == 2
    assert XgmiCost.calibrated(2, path=out) == XgmiCost(2)
    print("same-GPU fit:", {k: v for k, v in f.items() if k != "samples"})


@pytest.mark.parametrize("world", [2, 3])
def test_module_ddp_prescale_sum_bitwise(world):
    """module-path DDP averages like torch DDP - prescale by 1/world, then a
    SUM in fixed rank order - bitwise against a CPU oracle, at world 2 and at 3 (where
    sum-then-scale differs in the last bit)."""
    from ddp_amd.parallel import free_port

    res = _run(_module_grad_worker, world, free_port())
    assert all(r[1] == "ok" for r in res), res


def _plan_worker(rank, world, port, q, cap_mb, first_mb, dtype):
    try:
        _init(rank, world, port)
        import hashlib

        from ddp_amd.data import DeviceMNIST, synthetic_mnist
        from ddp_amd.engine import EngineOptions, FusedSimpleCNNEngine
        from ddp_amd.models import SimpleCNN
        from ddp_amd.models.layers import flat_space
        from ddp_amd.ops import FusedSGD

        torch.manual_seed(0)
        model = SimpleCNN().cuda()
        fs = flat_space(model)
        opt = FusedSGD(model, lr=0.05, momentum=0.9)
        imgs, labels = synthetic_mnist(4096)
        eo = EngineOptions(graph_steps=4, comm="xgmi", bucket_cap_mb=cap_mb, first_bucket_mb=first_mb,
                           dtype=dtype, bucket_plan="torch")
        eng = FusedSimpleCNNEngine(model, opt, DeviceMNIST(imgs, labels, torch.device("cuda", 0)),
                                   16, world, rank, None, eo)
        assert eng.comm_kind in ("xgmi", "xgmi1"), eng.comm_kind
        nb = eng.eng.num_buckets
        stages = [eng.eng.bucket_stage(b) for b in range(nb)]
        eng.refresh()
        eng.run_steps(6)  # 1 momentum-init step + a 4-step graph replay + 1 eager step
        eng.synchronize()
        p = fs.params.detach().cpu()
        allp = [None] * world
        dist.all_gather_object(allp, p)
        same = all(torch.equal(allp[r], allp[0]) for r in range(world))
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok" if same and torch.isfinite(p).all() else "ranks differ", nb, stages,
               hashlib.sha256(p.numpy().tobytes()).hexdigest()))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e), None, None, None))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine_any_bucket_plan_bitwise(dtype):
    """the fused engine takes ANY DDP bucket plan (--bucket_cap_mb):
    2, 3, 4 and 6 buckets at 2 ranks.  Every bucket is all-reduced (with the fused SGD) as
    soon as its gradients are final: fc-only buckets after fc_bwd, the rest after the conv
    backward.  The xGMI sum order is per element (fixed rank order), so every plan must
    give bit-identical parameters - across ranks and across plans."""
    from ddp_amd.parallel import free_port

    plans = [(25.0, 1.0, 2), (0.01, 1.0, 3), (0.05, 1e-6, 4), (1e-6, 1e-6, 6)]
    digests = set()
    for cap, first, want_nb in plans:
        res = _run(_plan_worker, 2, free_port(), cap, first, dtype)
        assert all(r[1] == "ok" for r in res), [r[:2] for r in res]
        nb, stages = res[0][2], res[0][3]
        assert nb == want_nb, (cap, first, nb)
        assert stages[0] == 0 and stages[-1] == 1, stages  # fc first, conv last
        digests.add(res[0][4])
        digests.add(res[1][4])
    assert len(digests) == 1, "bucket plans changed the parameters"


def _resnet_worker(rank, world, port, q, graph, bcast=None):
    try:
        _init(rank, world, port)
        from ddp_amd.models import resnet18
        from ddp_amd.models.layers import flat_space
        from ddp_amd.ops import CrossEntropyLoss, FusedSGD
        from ddp_amd.parallel import DistributedDataParallel

        dev = torch.device("cuda", 0)
        torch.manual_seed(0)
        model = resnet18(num_classes=10).to(dev)
        # gloo control plane -> the module reducer's data plane is the direct xGMI kernels
        ddp = DistributedDataParallel(model, bucket_cap_mb=8.0,
                                      broadcast_buffers=(not graph) if bcast is None else bcast)
        assert ddp.comm_kind == "xgmi", ddp.comm_kind
        nb = len(ddp.buckets)
        opt = FusedSGD(model, lr=0.05, momentum=0.9)
        lossf = CrossEntropyLoss()
        gens = [torch.Generator().manual_seed(100 * s + r) for s in range(3) for r in range(world)]
        batches = [(torch.randn(4, 3, 64, 64, generator=g).to(dev), torch.randint(0, 10, (4,), generator=g).to(dev))
                   for g in gens]  # batches[s * world + r]: step s, rank r

        def step(x, y):
            opt.zero_grad()
            loss = lossf(ddp(x), y)
            loss.backward()
            opt.step()
            return loss

        if graph:
            from ddp_amd.engine import GraphedStep

            gs = GraphedStep(step, batches[rank], warmup=1)  # step 0 (eager warm-up)
            torch.cuda.synchronize()
            dist.barrier()  # both ranks captured: replay in step (barrier spins are bounded)
            gs(*batches[world + rank])                         # steps 1, 2 replayed
            gs(*batches[2 * world + rank])
        else:
            for s in range(3):
                step(*batches[s * world + rank])
        torch.cuda.synchronize()
        xflags = ddp._native.xgmi.error_flags()
        p = flat_space(model).params.detach().cpu()
        allp = [None] * world
        dist.all_gather_object(allp, p)
        same = all(torch.equal(allp[r], allp[0]) for r in range(world))
        err = None
        if rank == 0:
            # DDP semantics on one process: per-rank gradients averaged (BatchNorm uses each
            # rank's own batch statistics), then the same optimizer step
            torch.manual_seed(0)
            ref = resnet18(num_classes=10).to(dev)
            fs = flat_space(ref)
            ropt = FusedSGD(ref, lr=0.05, momentum=0.9)
            for s in range(3):
                acc = torch.zeros_like(fs.grads)
                for r in range(world):
                    ropt.zero_grad()
                    lossf(ref(batches[s * world + r][0]), batches[s * world + r][1]).backward()
                    acc += fs.grads
                fs.grads.copy_(acc / world)
                ropt.step()
            torch.cuda.synchronize()
            pr = fs.params.detach().cpu()
            err = ((pr - p).norm() / pr.norm()).item()
            errs = [((pr - allp[r]).norm() / pr.norm()).item() for r in range(world)]
            if not same:
                print(f"[diag] per-rank rel err vs reference: {errs}", flush=True)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok" if same and not xflags else f"ranks differ (xgmi error flags {xflags})", nb, err))
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, repr(e) + traceback.format_exc()[-600:], None, None))


@pytest.mark.parametrize("graph,bcast", [(False, None), (False, False), (True, None)])
def test_resnet_ddp_two_ranks_xgmi(graph, bcast):
    """VERDICT r1 item 4 (BASELINE config 5 path): ResNet-18 under our DDP at 2 ranks on
    one GPU (gloo bootstrap, xGMI data plane in the native module reducer, several
    buckets): parameters bit-identical across ranks after 3 steps, equal to the
    one-process emulation of DDP's averaged gradients; graph=True replays the whole
    multi-rank step (forward, backward with the bucket all-reduces, optimizer) from one
    hipGraph."""
    from ddp_amd.parallel import free_port

    res = _run(_resnet_worker, 2, free_port(), graph, bcast)
    assert all(r[1] == "ok" for r in res), [r[:2] for r in res]
    r0 = [r for r in res if r[0] == 0][0]
    assert r0[2] >= 2, "expected several gradient buckets"
    assert r0[3] < 1e-5, f"2-rank DDP vs averaged single-process gradients: rel err {r0[3]:.2e}"
