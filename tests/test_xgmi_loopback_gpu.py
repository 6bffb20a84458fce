"""The xGMI all-reduce kernel body at every world size 1..8, on one GPU in one process.

C.XgmiLoopback runs N virtual ranks of one channel in ONE launch (xgmi_allreduce_group): every
rank's blocks run xgmi_allreduce_body from arguments filled like XgmiComm's and meet the other
ranks' blocks at the body's own barriers.  The cases (tests/xgmi_cases.py; their coverage of the
kernel's index plan is asserted in tests/test_xgmi_plan_cpu.py) run two-shot, two-shot with the
publish pass and a prescale, and one-shot, each with the plain and the write-through (WT) build,
three calls per run (both stage parities; a second data set of mixed magnitudes on the odd call).

Every buffer a kernel may write sits between sentinel bands; stages and shadow targets start as
NaN.  Checked bit for bit: the reduced bucket on every rank against the float32 sum in the
kernel's documented order (and within (N + 1) u sum|x| of the float64 sum), everything outside
the bucket, each rank's stage at the call's parity, the fused SGD's parameters / momentum /
shadows against C.sgd on the reduced gradient, the call counters, step counters and error word;
one-shot = two-shot and WT = plain.

What this does not show - visibility over real links and IPC mappings, skew between ranks across
calls, the timeout path, the pair kernel's completion count - stays with tests/test_xgmi_gpu.py.
Run with -s for the XGMI_LOOP <N> <case> ok lines."""
import numpy as np
import pytest
import torch

import xgmi_cases as X
from ddp_amd.ops import kernel_bounds as K
from elementwise import BF, F32, U, bits
from elementwise import Guarded as _Guarded

pytestmark = pytest.mark.gpu
dev = "cuda"
WORLDS = list(range(1, X.MAX_RANKS + 1))
SGD_OPTS = {
    "plain": dict(lr=0.05),
    "momentum": dict(lr=0.05, momentum=0.9),
    "nesterov_wd": dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-2),
    "dampening_wd": dict(lr=0.03, momentum=0.8, dampening=0.3, weight_decay=5e-3),
}
SCALES = (1.0, 1.0 / 3.0, 0.5)


def Guarded(n, dtype=F32, fill=None):  # (this file's bands are 2048 elements wide)
    return _Guarded(n, dtype, fill, guard=2048)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def inputs(case, idx, k):
    """Every rank's data buffer for call k (float32 [N][numel]): normal values, and on odd calls
    magnitudes from 1e-3 to 1e3."""
    numel = case.off + case.n + case.pad
    g = np.random.default_rng(100_000 * case.N + 100 * idx + k)
    x = g.standard_normal((case.N, numel))
    if k % 2:
        x = np.sign(x) * 10.0 ** g.uniform(-3.0, 3.0, size=x.shape)
    return x.astype(np.float32)


def shadow_regions(case, k):
    """(off, n, kind, a, b, c) of call k's shadows, at most MAX_SHADOWS; all six kinds over the
    three calls.  Regions start and end inside the bucket off quad borders, reach out of the
    bucket on both sides, and (4-aligned ones of a 4-aligned bucket) take the vector stores."""
    off, n = case.off, case.n
    end, numel = off + n, off + n + case.pad
    al = off + (-off) % 4
    lo = max(off - 3, 0)
    if n >= 700:
        sets = [[(off + 2, 9, K.SHADOW_BF16, 0, 0, 0), (off + 13, 27, K.SHADOW_BF16_TAPT, 3, 9, 1),
                 (off + 41, 256, K.SHADOW_BF16_FCFRAG, 16, 16, 0), (off + 323, 21, K.SHADOW_BF16_PAD4, 0, 0, 0)],
                [(off + 6, 27, K.SHADOW_F32_TAPT, 3, 9, 1), (al + 64, 512, K.SHADOW_F32_FCFRAG, 16, 16, 0),
                 (lo, 10, K.SHADOW_BF16, 0, 0, 0), (end - 6, numel - (end - 6), K.SHADOW_BF16, 0, 0, 0)],
                [(al + 8, 64, K.SHADOW_BF16, 0, 0, 0), (al + 128, 256, K.SHADOW_BF16_FCFRAG, 16, 16, 0),
                 (off + 401, 256, K.SHADOW_F32_FCFRAG, 16, 16, 0),
                 (end - 10, 12 if case.pad >= 2 else 9, K.SHADOW_BF16_PAD4, 0, 0, 0)]]
    else:
        wide = (lo, numel - lo, K.SHADOW_BF16, 0, 0, 0)
        sets = [[wide],
                [(off, n, K.SHADOW_F32_TAPT, n, 1, 1)] + ([(off + 1, (n - 1) // 3 * 3, K.SHADOW_BF16_PAD4, 0, 0, 0)]
                                                         if n >= 4 else []),
                [wide, (off, n, K.SHADOW_BF16_TAPT, 1, n, 1)]]
    regs = sets[k % 3]
    assert len(regs) <= X.MAX_SHADOWS and all(o >= 0 and o + rn <= numel for o, rn, *_ in regs)
    return regs


def shadow_dsts(regs):
    return [Guarded(K.shadow_dst_numel(kind, rn), F32 if K.shadow_is_f32(kind) else BF) for _, rn, kind, *_ in regs]


class Reference:
    """What every rank must hold after each call of a case at one prescale: computed once (numpy
    float32 in the kernel's order; C.sgd on the reduced gradient) and shared by the two-shot,
    one-shot, plain and WT runs, which must all give these bits."""

    def __init__(self, C, case, idx, ps):
        self.C, self.case, self.idx, self.ps = C, case, idx, ps
        self.scale = SCALES[idx % len(SCALES)]
        self.calls = []
        numel = case.off + case.n + case.pad
        self.p0 = torch.from_numpy(np.random.default_rng(7 + idx).standard_normal(numel).astype(np.float32))
        self.p = self.p0.clone().to(dev)
        self.m = torch.full((numel,), float("nan"), device=dev)

    def call(self, k):
        while len(self.calls) <= k:
            self.calls.append(self._next(len(self.calls)))
        return self.calls[k]

    def _next(self, k):
        case, N, off, n = self.case, self.case.N, self.case.off, self.case.n
        x = inputs(case, self.idx, k)
        pre = x[:, off:off + n] * np.float32(self.ps)       # each rank's value, rounded once
        acc = pre[0].copy()
        for r in range(1, N):
            acc = acc + pre[r]                               # rank order, float32
        want = acc * np.float32(self.scale)
        assert pre.dtype == acc.dtype == want.dtype == np.float32
        # the replay itself against float64: (N + 1) roundings of magnitudes <= sum |x ps|
        x64 = x[:, off:off + n].astype(np.float64) * float(np.float32(self.ps))
        ref64 = x64.sum(0) * float(np.float32(self.scale))
        bound = (N + 1) * U * np.abs(x64).sum(0) * abs(float(np.float32(self.scale)))
        assert np.all(np.abs(want.astype(np.float64) - ref64) <= bound), f"{case.name}: replay outside its bound"
        out = dict(x=x, pre=pre, acc=acc, want=want, ref64=ref64, bound=bound)
        if case.sgd:
            o = SGD_OPTS[case.sgd]
            mom = o.get("momentum", 0.0)
            regs = shadow_regions(case, k)
            dsts = shadow_dsts(regs)
            g = torch.zeros_like(self.p)
            g[off:off + n] = torch.from_numpy(want).to(dev)
            p_after, m_after = self.p.clone(), self.m.clone()
            self.C.sgd(p_after, g, m_after if mom else None, o["lr"], mom, o.get("dampening", 0.0),
                       o.get("weight_decay", 0.0), o.get("nesterov", False), False, mom != 0.0 and k == 0, True,
                       [(so, rn, d.t, kind, a, b, c) for (so, rn, kind, a, b, c), d in zip(regs, dsts)])
            torch.cuda.synchronize()
            # the fused optimizer touches the bucket only
            self.p[off:off + n] = p_after[off:off + n]
            if mom:
                self.m[off:off + n] = m_after[off:off + n]
            sh = []
            for (so, rn, kind, a, b, c), d in zip(regs, dsts):
                ix = torch.from_numpy(K.shadow_index(kind, rn, a, b, c))
                j0, j1 = max(0, off - so), min(rn, off + n - so)
                assert j0 < j1, "a shadow region outside the bucket"
                e = torch.full((d.t.numel(),), float("nan"), dtype=d.t.dtype)
                e[ix[j0:j1]] = d.t.cpu()[ix[j0:j1]]
                sh.append(e)
            out.update(p=self.p.cpu().clone(), m=self.m.cpu().clone(), sh=sh, regs=regs)
        return out


class World:
    """One XgmiLoopback per world size; a two-shot and a one-shot channel per case, their stage
    buffers guarded, made once."""

    def __init__(self, C, N):
        self.C, self.N = C, N
        self.lb = C.XgmiLoopback(N, 0)
        self.cases = X.cases(N)
        self.chan, self.count, self.refs = {}, {}, {}
        for case in self.cases:
            for oneshot in (False, True):
                sf = C.xgmi_stage_floats(case.n, N, oneshot)
                assert sf == X.stage_floats(case.n, N, oneshot)
                stages = [Guarded(2 * sf) for _ in range(N)]
                ch = self.lb.add_channel(case.off, case.n, oneshot, case.cap, [s.t for s in stages])
                assert self.lb.slice(ch) == X.slice_len(case.n, N), case.name
                assert self.lb.blocks(ch) == X.blocks(case.n, N, oneshot, case.cap), case.name
                self.chan[case.name, oneshot] = (ch, stages)
                self.count[ch] = 0

    def ref(self, case, idx, ps):
        key = (case.name, ps)
        if key not in self.refs:
            self.refs[key] = Reference(self.C, case, idx, ps)
        return self.refs[key]


_worlds = {}


def world(C, N):
    if N not in _worlds:
        _worlds[N] = World(C, N)
    return _worlds[N]


def run(w, case, idx, oneshot, publish, ps, wt):
    """`calls` calls of one channel in one mode, every check after every call."""
    N, off, n = case.N, case.off, case.n
    numel = off + n + case.pad
    lb, ref = w.lb, w.ref(case, idx, ps)
    ch, stages = w.chan[case.name, oneshot]
    sl, sf, nblk = lb.slice(ch), X.stage_floats(n, N, oneshot), lb.blocks(ch)
    what0 = f"N={N} {case.name} {'one' if oneshot else 'two'}-shot publish={publish} ps={ps:.3g} wt={wt}"
    opts = SGD_OPTS.get(case.sgd)
    mom = opts.get("momentum", 0.0) if opts else 0.0
    data = [Guarded(numel) for _ in range(N)]
    step = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(N)]
    params = mbuf = None
    if opts:
        params = [Guarded(numel) for _ in range(N)]
        for p in params:
            p.t.copy_(ref.p0)
        if mom:
            mbuf = [Guarded(numel) for _ in range(N)]
    for k in range(case.calls):
        what = f"{what0} call {k}"
        want = ref.call(k)
        for r in range(N):
            data[r].t.copy_(torch.from_numpy(want["x"][r]))
            lb.set_data(r, data[r].t)
        for s in stages:
            s.t.fill_(float("nan"))
        kw, dsts = {}, None
        if opts:
            dsts = [shadow_dsts(want["regs"]) for _ in range(N)]
            kw = dict(params=[p.t for p in params], momentum_buffer=[m.t for m in mbuf] if mom else None,
                      shadows=[[(so, rn, d.t, kind, a, b, c) for (so, rn, kind, a, b, c), d in zip(want["regs"], ds)]
                               for ds in dsts],
                      first_step=mom != 0.0 and k == 0, **opts)
        torch.cuda.synchronize()
        lb.all_reduce(ch, scale=ref.scale, publish=publish, prescale=ps, wt=wt, step_ctr=step, **kw)
        torch.cuda.synchronize()
        w.count[ch] += 1
        e = w.count[ch]
        assert lb.error_flags() == 0, f"{what}: error word {lb.error_flags():#x}"
        for r in range(N):
            got = data[r].t.cpu().numpy()
            # ---- the reduced bucket, and nothing else
            gb = got[off:off + n]
            assert not np.isnan(gb).any(), f"{what} rank {r}: NaN in the bucket"
            if not np.array_equal(gb.view(np.int32), want["want"].view(np.int32)):
                bad = np.flatnonzero(gb.view(np.int32) != want["want"].view(np.int32))
                raise AssertionError(f"{what} rank {r}: {bad.size} of {n} elements differ from the rank-order sum, "
                                     f"first {bad[:6].tolist()} got {gb[bad[:3]]} want {want['want'][bad[:3]]}")
            assert np.all(np.abs(gb.astype(np.float64) - want["ref64"]) <= want["bound"]), f"{what} rank {r}: float64 bound"
            x = want["x"][r]
            assert np.array_equal(got[:off].view(np.int32), x[:off].view(np.int32)), f"{what} rank {r}: wrote before the bucket"
            assert np.array_equal(got[off + n:].view(np.int32), x[off + n:].view(np.int32)), f"{what} rank {r}: wrote behind the bucket"
            data[r].check(f"{what} data[{r}]")
            # ---- the stage at this call's parity; the other parity and the rest stay NaN
            exp = np.full(2 * sf, np.nan, dtype=np.float32)
            base = (e & 1) * sf
            if oneshot:
                exp[base:base + (n + 3) // 4 * 4] = 0.0
                exp[base:base + n] = want["pre"][r]
            else:
                assert sf == sl
                lim = min(sl, n - r * sl)
                if lim > 0:
                    exp[base:base + (lim + 3) // 4 * 4] = 0.0
                    exp[base:base + lim] = want["acc"][r * sl:r * sl + lim]
            assert same(stages[r].t, exp), f"{what} rank {r}: stage"
            stages[r].check(f"{what} stage[{r}]")
            assert int(step[r].item()) == k + 1, f"{what} rank {r}: step counter {int(step[r].item())}"
            # ---- fused SGD: C.sgd on the reduced gradient, the same on every rank
            if opts:
                assert same(params[r].t, want["p"]), f"{what} rank {r}: parameters"
                params[r].check(f"{what} params[{r}]")
                if mom:
                    assert same(mbuf[r].t, want["m"]), f"{what} rank {r}: momentum"
                    mbuf[r].check(f"{what} mbuf[{r}]")
                for d, es, reg in zip(dsts[r], want["sh"], want["regs"]):
                    assert same(d.t, es), f"{what} rank {r}: shadow {reg}"
                    d.check(f"{what} shadow {reg}")
    for r in range(N):
        for b in range(nblk):
            assert lb.seq(ch, r, b) == w.count[ch], f"{what0}: call counter of rank {r} block {b}"


@pytest.mark.parametrize("idx", range(max(len(X.cases(N)) for N in WORLDS)))
@pytest.mark.parametrize("N", WORLDS)
def test_loopback_allreduce(C, N, idx):
    w = world(C, N)
    if idx >= len(w.cases):
        return  # (this world size has fewer distinct small lengths)
    case = w.cases[idx]
    # every mode checks against the one reference of its prescale: one-shot = two-shot and
    # WT = plain bit for bit, in the bucket, the parameters, the momentum and the shadows
    for oneshot, publish, ps in X.modes(case):
        for wt in (False, True):
            run(w, case, idx, oneshot, publish, ps, wt)
    print(f"XGMI_LOOP {N} {case.name} ok")


def test_binding_refuses_what_could_spin(C):
    """Every block of every virtual rank must be resident at once: world * blocks <= 64; stages
    too small, a bucket outside the data buffer and a prescale without a publish pass are refused
    before any launch."""
    lb = C.XgmiLoopback(8, 0)
    n = 8 * 4 * 256 * 9
    st = [torch.zeros(2 * C.xgmi_stage_floats(n, 8, False), device=dev) for _ in range(8)]
    with pytest.raises(RuntimeError, match="world \\* blocks"):
        lb.add_channel(0, n, False, 0, st)          # 9 blocks x 8 ranks
    with pytest.raises(RuntimeError, match="world \\* blocks"):
        lb.add_channel(0, n, False, 9, st)
    with pytest.raises(RuntimeError, match="stage"):
        lb.add_channel(0, n, False, 8, [s[:-4] for s in st])
    with pytest.raises(RuntimeError):
        lb.add_channel(0, n, False, 8, st[:7])
    ch = lb.add_channel(0, n, False, 8, st)
    assert lb.blocks(ch) == 8 and lb.slice(ch) == n // 8
    with pytest.raises(RuntimeError, match="outside the data buffer"):
        lb.all_reduce(ch)                           # no data yet
    data = [torch.zeros(n, device=dev) for _ in range(8)]
    for r in range(8):
        lb.set_data(r, data[r][:n - 4])
    with pytest.raises(RuntimeError, match="outside the data buffer"):
        lb.all_reduce(ch)
    for r in range(8):
        lb.set_data(r, data[r])
    with pytest.raises(RuntimeError, match="prescale"):
        lb.all_reduce(ch, prescale=0.5)
    with pytest.raises(RuntimeError):
        lb.seq(ch, 0, 8)
    with pytest.raises(RuntimeError):
        C.XgmiLoopback(9, 0)
    assert lb.error_flags() == 0 and lb.seq(ch, 0, 0) == 0
