"""One ResNet-18 training step on the module path, stage by stage and element by element, against
float64 (tests/test_resnet_step_elementwise_gpu.py records the step on the GPU and runs it
through ``check_step``; tests/test_resnet_step_bounds_cpu.py shows that ``check_step`` admits a
correct step and rejects wrong ones).  A helper module, not a test module; it needs no GPU.

Recording.  ``Recorder`` wraps the native module: every kernel call of ``KERNELS`` is kept as a
``Call`` - the name, the arguments with every tensor cloned to the CPU before the call (``a`` /
``kw``) and the same tensors cloned after it (``o`` / ``ko``).  Everything else (plan queries) is
forwarded untouched.  ``parse_trace`` walks this file's OWN description of ResNet-18
(``topology``: stem, max pool, eight basic blocks with their strides and three downsamples,
average pool, head; which tensor feeds which; which gradients sum at a block input) and takes
the calls it expects from the trace, in order; a missing, extra or reordered call is an
``OrderError`` that names the layer.

Checking.  ``check_step`` is teacher-forced: the float64 reference of a stage is computed on the
CPU from the tensors the step stored for the stage before it - the tensor the TOPOLOGY says
feeds the stage, not the one the call happened to receive - so errors do not compound, every
bound is the one-kernel bound and a wiring error fails at its own stage.  ReLU masks come from
the recorded bn_apply output.  No element is excluded and nothing is calibrated on the kernels.

Bounds.  u = 2**-24, n = accumulated terms of one output element, A = the same operation on the
operands' absolute values, P = N OH OW pixels of a BatchNorm.  The formulae are the ones of
tests/test_resnet_geometry_gpu.py (convolutions), tests/test_resnet_ops_elementwise_gpu.py
(BatchNorm apply / backward, pools, head GEMMs, cross-entropy), tests/label_smoothing_cases.py
(smoothed cross-entropy) and ddp_amd/ops/kernel_bounds.py (grad_reduce, SGD):

  weight_bf16   the MFMA operand is, bit for bit, bf16(master parameter before the step)
  pad4          the stem's operand [64,7,7,4]: channels 0..2 as above, channel 3 exactly 0
  conv_y        bf16 out: 2**-8 |ref| + 2 n u A, n = KH KW Cin (stem: 147)
  stats         slab summed over its rows vs the stored y: 2 P u sum|y|, 2 P u sum y^2; the
                slab bn_finalize read is the slab the convolution wrote (bit for bit)
  mean, invstd, running_mean, running_var: ``bn_finalize_bounds`` below; nbt: exact
  bn_apply      2**-8 |ref| + 4 u (|x sc| + |mean sc| + |beta| + |res|), sc = invstd gamma; the
                residual and the ReLU flag are the topology's
  maxpool       y and argmax bit for bit (R.maxpool64)
  avgpool       2 (HW + 1) u sum|x| / HW
  head, head_dx, head_dw, head_db:  2 (2 K + 3) u (|A| |B| + |bias| + |prior|)
  loss, dlogits no smoothing: g (p (2 D + 64) u + 2 u) and mean (D + 64) u max(1, |row|);
                smoothing: label_smoothing_cases.bounds.  g = fl32(1 / B) is part of the reference
  avgpool_bwd   (2**-8 + 2 u) |ref|
  bn_bwd_dres   d = bf16(d1 + d2) (bn_bwd_reduce_kernel / bn_bwd_apply_kernel round the sum of the
                two upstream gradients to bf16 as they load it, unpack8_sum, BEFORE the mask and
                before anything is accumulated - reproduced exactly on the CPU, so the sum needs
                no bound), masked by the stored output > 0: bit for bit.  d1 / d2 are what the
                topology says: at a block input the conv1 branch's dx plus dres of bn2 (identity
                block) or dx of the downsample conv
  bn_dgamma,    E_q = 2 (P + 3) u sum|d xhat|, E_d = 2 P u sum|d|; with a prior (accumulation)
  bn_dbeta      2 (P + 4) u (sum|d xhat| + |prior|), 2 (P + 1) u (sum|d| + |prior|)
  bn_bwd_dy     2**-8 |ref| + |k| [6 u (P |d| + |S_d| + |xhat S_q|) + E_d + |xhat| E_q]
  dgrad         bf16 out, n = KH KW Cout; none for the stem (a dgrad call there is an OrderError)
  wgrad_slab    row r = output pixels [r ppc, (r + 1) ppc): 2 ppc u A_r
  wgrad         one chunk: 2 n u A, n = P (+ 1 and A + |prior| with a prior); chunked: the
                float64 sum of the STORED rows (+ prior) within kernel_bounds.reduce_bound
  maxpool_bwd   d = bf16(dy + stash), routed by the stored argmax, summed in fp32 in window
                order, one bf16 rounding: bit for bit
  landing       over the whole flat gradient buffer the optimizer read: every parameter's view
                is bit for bit the output of the stage that produced it; every element outside
                all views kept its bits
  param,        R.sgd64 of the flat buffers the optimizer read: kernel_bounds.sgd_bounds
  momentum
  shadow_bf16,  the flat bf16 copy / the PAD4 copy after the step are bit for bit bf16(new
  shadow_pad4   parameters) (PAD4: channel 3 exactly 0)

``bn_finalize_bounds`` (bn_finalize_kernel, derived from its arithmetic; S, Q the float64 column
sums of the slab, S_A, Q_A of its absolute values, m = S / P, v = max(Q / P - m^2, 0)):

  sums          each column is added in fp32 in some fixed tree of at most `rows` leaves per
                level: dS = 2 rows u S_A, dQ = 2 rows u Q_A
  mean          fl(S' / P): dm = dS / P + u (|m| + dS / P)
  var           fl(fl(Q' / P) - fl(mean mean)) (or one fma), clamped at 0 (1-Lipschitz, the
                reference clamps too): three roundings, each at most u times a value that
                Q / P + m^2 dominates:  dv = dQ / P + 2 |m| dm + dm^2 + 3 u (Q / P + m^2 + dQ / P)
  invstd        rsqrtf(fl(var + eps)): the argument is within da = dv + u (v + eps + dv) of
                v + eps and, being clamped, never below eps (1 - u).  By the mean value theorem
                |rsqrt(a') - rsqrt(a)| <= 1/2 i_lo^3 da with i_lo = rsqrt(max(a - da, eps (1 - u))),
                the inverse deviation at the interval's worst point; rsqrtf itself is good to
                1 ulp (2 u relative), one more u of slack: di = 1/2 i_lo^3 da + 3 u i_lo.
                Where m^2 >> v (a channel of mean 8, deviation 2**-6: 3 u m^2 is 5 % of v) da is
                a sizeable fraction of v and the bound says so - it is what fp32 allows
  running_mean  fl(fl(a rm) + fl(mom mean)) with a = fl32(1 - mom) taken as the kernel's constant:
                three roundings: mom dm + 3 u (|a rm| + |mom m| + mom dm)
  running_var   unb = fl(fl(var P) / (P - 1)) for P > 1, var for P = 1: with f = P / (P - 1) (or 1)
                du = f dv + 2 u f (v + dv);  then as the mean: mom du + 3 u (|a rv| + mom (f v + du))

``emulate`` is a plain fp32 / bf16 model of the step that follows ``topology`` (torch's float32
operators, bf16 roundings at the kernels' store points) and emits a trace in the recorder's
format; ``plant=`` plants one wiring error (tests/test_resnet_step_bounds_cpu.py).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import elementwise as EW
import label_smoothing_cases as LS
from ddp_amd.ops import kernel_bounds as K
from ddp_amd.ops import reference as R
from elementwise import BF, INF, U, bf, bits, bitwise, f64, n32, nchw, nhwc, worst  # noqa: F401  (reachable as S.worst ...)

BN_EPS, BN_MOM = 1e-5, 0.1
KERNELS = {"conv_gemm_fwd", "bn_finalize", "bn_apply", "maxpool_fwd", "avgpool_fwd", "sgemm", "xent", "bn_bwd",
           "conv_gemm_dgrad", "conv_gemm_wgrad", "grad_reduce", "maxpool_bwd", "avgpool_bwd", "sgd"}
# the order the stages depend on each other in: a planted error is "caught at its stage" when
# that stage is the first of these that fails
STAGES = ("order", "weight_bf16", "pad4", "conv_y", "stats", "mean", "invstd", "running_mean", "running_var", "nbt",
          "bn_apply", "maxpool", "avgpool", "head", "loss", "dlogits", "head_dx", "head_dw", "head_db", "avgpool_bwd",
          "bn_bwd_dres", "bn_dgamma", "bn_dbeta", "bn_bwd_dy", "dgrad", "wgrad_slab", "wgrad", "maxpool_bwd",
          "landing", "param", "momentum", "shadow_bf16", "shadow_pad4")
failing = functools.partial(EW.failing, order=STAGES)                       # failing(res)
report = functools.partial(EW.report, order=STAGES, tag="RESNET_STEP_RATIO")  # report(res, case)


# ------------------------------------------------------------------------------- topology
def topology():
    """ResNet-18 as this file sees it.  ``convs``: every conv + BatchNorm in forward order -
    name (its weight is ``name + ".weight"``), bn, kernel k / stride s / pad p, cin / cout, ``src``
    (the tensor it reads: "img", "pool" or a conv's name = that conv's BatchNorm output), ``res``
    (the tensor its BatchNorm adds) and ``relu``.  ``blocks``: name, ``src`` (the block input), ``ds``.
    ``grad``: conv -> (first, second) upstream gradient of its BatchNorm, each ("avgpool" | "dx"
    | "dres" | "maxpool", producer)."""
    convs = [dict(name="conv1", bn="bn1", k=7, s=2, p=3, cin=3, cout=64, src="img", res=None, relu=True, role="stem")]
    blocks, grad = [], {}
    cin, src = 64, "pool"
    for li, cout in enumerate((64, 128, 256, 512), 1):
        for j in range(2):
            s = 2 if (j == 0 and li > 1) else 1
            b = f"layer{li}.{j}"
            ds = s != 1 or cin != cout
            convs.append(dict(name=b + ".conv1", bn=b + ".bn1", k=3, s=s, p=1, cin=cin, cout=cout, src=src, res=None,
                              relu=True, role="conv1"))
            if ds:
                convs.append(dict(name=b + ".downsample.0", bn=b + ".downsample.1", k=1, s=s, p=0, cin=cin, cout=cout,
                                  src=src, res=None, relu=False, role="ds"))
            convs.append(dict(name=b + ".conv2", bn=b + ".bn2", k=3, s=1, p=1, cin=cout, cout=cout, src=b + ".conv1",
                              res=b + ".downsample.0" if ds else src, relu=True, role="conv2"))
            blocks.append(dict(name=b, src=src, ds=ds))
            cin, src = cout, b + ".conv2"
    for i, b in enumerate(blocks):
        n = b["name"]
        if i + 1 < len(blocks):
            nb = blocks[i + 1]
            second = ("dx", nb["name"] + ".downsample.0") if nb["ds"] else ("dres", nb["name"] + ".conv2")
            grad[n + ".conv2"] = (("dx", nb["name"] + ".conv1"), second)
        else:
            grad[n + ".conv2"] = (("avgpool", None), None)
        grad[n + ".conv1"] = (("dx", n + ".conv2"), None)
        if b["ds"]:
            grad[n + ".downsample.0"] = (("dres", n + ".conv2"), None)
    b0 = blocks[0]["name"]
    grad["pool"] = (("dx", b0 + ".conv1"), ("dres", b0 + ".conv2"))
    grad["conv1"] = (("maxpool", None), None)
    return dict(convs=convs, blocks=blocks, grad=grad)


TOPO = topology()
CONV = {c["name"]: c for c in TOPO["convs"]}


def param_names():
    """Registration order of the parameters (the flat space lays them out in reverse)."""
    out = []
    for c in TOPO["convs"]:
        if c["role"] == "ds":  # (registered after bn2)
            continue
        out += [c["name"] + ".weight", c["bn"] + ".weight", c["bn"] + ".bias"]
        if c["role"] == "conv2":
            d = CONV.get(c["name"][:-5] + "downsample.0")
            if d:
                out += [d["name"] + ".weight", d["bn"] + ".weight", d["bn"] + ".bias"]
    return out + ["fc.weight", "fc.bias"]


def flat_layout(shapes, align=64):
    """{name: (offset, numel)} and the buffer's length, reverse registration order."""
    off, lay = 0, {}
    for n in reversed(param_names()):
        ne = int(np.prod(shapes[n]))
        lay[n] = (off, ne)
        off += (ne + align - 1) // align * align
    return lay, off


# ------------------------------------------------------------------------------- recording
class Call:
    __slots__ = ("name", "a", "o", "kw", "ko")

    def __init__(self, name, a, o, kw=None, ko=None):
        self.name, self.a, self.o, self.kw, self.ko = name, list(a), list(o), kw or {}, ko or {}

    def __repr__(self):
        return f"Call({self.name})"


def snap(v):
    if isinstance(v, torch.Tensor):
        return v.detach().clone().cpu()
    if isinstance(v, (list, tuple)):
        return type(v)(snap(x) for x in v)
    if isinstance(v, dict):
        return {k: snap(x) for k, x in v.items()}
    return v


class Recorder:
    """A proxy around the native module that records the calls of ``kernels`` (None: ``KERNELS``).
    ``outputs`` {name: f(a, kw) -> the tensors the call must write in full}: each is filled with
    NaN before the launch, so that an element the kernel leaves unwritten shows in ``o``
    (tests/simplecnn_step_cases.py: the Functions there allocate their outputs with torch.empty)."""

    def __init__(self, native_module, kernels=None, outputs=None):
        self._native = native_module
        self._kernels = KERNELS if kernels is None else kernels
        self._outputs = outputs or {}
        self.trace = []

    def __getattr__(self, name):
        f = getattr(self._native, name)
        if name not in self._kernels:
            return f

        def call(*a, **kw):
            for t in self._outputs[name](a, kw) if name in self._outputs else ():
                t.fill_(float("nan"))
            pa, pk = snap(a), snap(kw)
            out = f(*a, **kw)
            self.trace.append(Call(name, pa, snap(a), pk, snap(kw)))
            return out

        return call


class OrderError(Exception):
    pass


class _Cursor:
    def __init__(self, trace, i=0):
        self.t, self.i = trace, i

    def peek(self):
        return self.t[self.i].name if self.i < len(self.t) else None

    def take(self, name, layer):
        got = self.peek()
        if got != name:
            raise OrderError(f"{layer}: expected {name} at call {self.i}, found {got}")
        self.i += 1
        return self.t[self.i - 1]


def parse_forward_backward(cur, materialise=None):
    """One forward + backward from the cursor.  ``materialise`` None: the materialised chain
    (every BatchNorm followed by its own bn_apply).  A dict {conv2 name: bool}: the deferred chain -
    the stem's and every conv1's BatchNorm has NO bn_apply of its own; a conv2 whose entry is True
    is preceded by exactly one materialising bn_apply of its input, one whose entry is False by none."""
    st = dict(fwd={}, bwd={}, mat={})
    deferred = materialise is not None
    for c in TOPO["convs"]:
        n = c["name"]
        if deferred and c["role"] == "conv2" and materialise[n]:
            st["mat"][c["src"]] = cur.take("bn_apply", n + " (materialising its input)")
        f = dict(conv=cur.take("conv_gemm_fwd", n), fin=cur.take("bn_finalize", c["bn"]), app=None)
        if not (deferred and c["role"] in ("stem", "conv1")):
            f["app"] = cur.take("bn_apply", c["bn"])
        st["fwd"][n] = f
        if c["role"] == "stem":
            st["maxpool"] = cur.take("maxpool_fwd", "maxpool")
    st["avgpool"] = cur.take("avgpool_fwd", "avgpool")
    st["head"] = cur.take("sgemm", "fc")
    st["xent"] = cur.take("xent", "loss")
    st["head_bwd"] = [cur.take("sgemm", "fc backward " + w) for w in ("dx", "dW", "db")]
    st["avgpool_bwd"] = cur.take("avgpool_bwd", "avgpool backward")
    for b in reversed(TOPO["blocks"]):
        for role in ("conv2", "downsample.0", "conv1"):
            n = b["name"] + "." + role
            if n in CONV:
                st["bwd"][n] = _parse_conv_bwd(cur, n, True)
    st["maxpool_bwd"] = cur.take("maxpool_bwd", "maxpool backward")
    st["bwd"]["conv1"] = _parse_conv_bwd(cur, "conv1", False)
    return st


def _parse_conv_bwd(cur, n, dgrad):
    d = dict(bn=cur.take("bn_bwd", CONV[n]["bn"] + " backward"), dgrad=None, red=None)
    if dgrad:
        d["dgrad"] = cur.take("conv_gemm_dgrad", n + " data gradient")
    d["wgrad"] = cur.take("conv_gemm_wgrad", n + " weight gradient")
    out = d["wgrad"].a[2]
    if out.dim() == 2:  # a slab [chunks][row]
        d["red"] = cur.take("grad_reduce", n + " slab reduction")
    return d


def parse_trace(trace, backwards=1, materialise=None):
    """[(forward + backward) x ``backwards``, then the optimizer] -> (list of step dicts, sgd Call)."""
    cur = _Cursor(trace)
    sts = [parse_forward_backward(cur, materialise) for _ in range(backwards)]
    sgd = cur.take("sgd", "optimizer")
    if cur.peek() is not None:
        raise OrderError(f"after the optimizer: {len(trace) - cur.i} extra calls, first {cur.peek()}")
    return sts, sgd


def stored(st):
    """{name: tensor} of everything a parsed forward + backward stored (the cross-chain
    bit-for-bit comparison runs over the names both chains have)."""
    out = {}
    for n, f in st["fwd"].items():
        out[n + "/y"], out[n + "/stats"] = f["conv"].o[3], f["conv"].o[9]
        for k, i in (("running_mean", 6), ("running_var", 7), ("mean", 8), ("invstd", 9), ("nbt", 10)):
            out[f"{n}/{k}"] = f["fin"].o[i]
        if f["app"] is not None:
            out[n + "/act"] = f["app"].o[7]
    for n, c in st["mat"].items():
        out[n + "/act"] = c.o[7]
    out["pool/y"], out["pool/argmax"] = st["maxpool"].o[1], st["maxpool"].o[2]
    out["avgpool"], out["logits"] = st["avgpool"].o[1], st["head"].o[9]
    out["dlogits"], out["loss"] = st["xent"].o[5], st["xent"].o[6]
    for k, c in zip(("head_dx", "fc.weight/grad", "fc.bias/grad"), st["head_bwd"]):
        out[k] = c.o[9]
    out["avgpool_bwd"] = st["avgpool_bwd"].o[1]
    for n, b in st["bwd"].items():
        out[n + "/dy"], out[n + "/dgamma"], out[n + "/dbeta"] = b["bn"].o[12], b["bn"].o[9], b["bn"].o[10]
        if b["bn"].o[13] is not None:
            out[n + "/dres"] = b["bn"].o[13]
        if b["dgrad"] is not None:
            out[n + "/dx"] = b["dgrad"].o[3]
        out[n + "/dw"] = _dw_out(b)
    out["pool/dx"] = st["maxpool_bwd"].o[2]
    return out


def _dw_out(b):
    return b["red"].o[0][0][5] if b["red"] is not None else b["wgrad"].o[2]


def produced_grads(st):
    """{parameter name: the tensor the producing stage left for it}."""
    g = {"fc.weight": st["head_bwd"][1].o[9], "fc.bias": st["head_bwd"][2].o[9]}
    for n, b in st["bwd"].items():
        g[n + ".weight"] = _dw_out(b)
        g[CONV[n]["bn"] + ".weight"], g[CONV[n]["bn"] + ".bias"] = b["bn"].o[9], b["bn"].o[10]
    return g


# ------------------------------------------------------------------------------- references
def conv_fwd(x, w, s, p, dtype=torch.float64):
    return nhwc(F.conv2d(nchw(x, dtype), nchw(w, dtype), stride=s, padding=p))


def conv_dgrad(xshape, w, dy, s, p, dtype=torch.float64):
    N, H, W, C = xshape
    return nhwc(torch.nn.grad.conv2d_input((N, C, H, W), nchw(w, dtype), nchw(dy, dtype), stride=s, padding=p))


def conv_wgrad(x, wshape, dy, s, p, dtype=torch.float64):
    O, KH, KW, I = wshape
    return nhwc(torch.nn.grad.conv2d_weight(nchw(x, dtype), (O, I, KH, KW), nchw(dy, dtype), stride=s, padding=p))


def chunk_of(dy, r, ppc):
    """dy with every output pixel outside the flattened range [r ppc, (r + 1) ppc) zeroed."""
    flat = dy.reshape(-1, dy.shape[-1])
    out = torch.zeros_like(flat)
    out[r * ppc:(r + 1) * ppc] = flat[r * ppc:(r + 1) * ppc]
    return out.view(dy.shape)


def bn_finalize_bounds(slab, count, eps, momentum, rm0=None, rv0=None):
    """Float64 references and a-priori bounds of bn_finalize for the slab [rows][2][C] it read
    (see the module docstring): {"mean": (ref, bound), "invstd": ..., "running_mean": ...,
    "running_var": ...}."""
    s = f64(slab)
    rows, P = s.shape[0], float(count)
    eps, mom = n32(eps), n32(momentum)
    a = float(np.float32(1.0) - np.float32(momentum))
    S, Q = s[:, 0].sum(0), s[:, 1].sum(0)
    dS, dQ = 2 * rows * U * s[:, 0].abs().sum(0), 2 * rows * U * s[:, 1].abs().sum(0)
    m = S / P
    v = (Q / P - m * m).clamp(min=0.0)
    dm = dS / P + U * (m.abs() + dS / P)
    dv = dQ / P + 2 * m.abs() * dm + dm * dm + 3 * U * (Q.abs() / P + m * m + dQ / P)
    arg = v + eps
    da = dv + U * (arg + dv)
    i_lo = (arg - da).clamp(min=eps * (1 - U)).rsqrt()
    out = {"mean": (m, dm), "invstd": (arg.rsqrt(), 0.5 * i_lo ** 3 * da + 3 * U * i_lo)}
    if rm0 is not None:
        rm0, rv0 = f64(rm0), f64(rv0)
        f = P / (P - 1.0) if P > 1.0 else 1.0
        du = f * dv + 2 * U * f * (v + dv)
        out["running_mean"] = (a * rm0 + mom * m, mom * dm + 3 * U * ((a * rm0).abs() + (mom * m).abs() + mom * dm))
        out["running_var"] = (a * rv0 + mom * f * v, mom * du + 3 * U * ((a * rv0).abs() + mom * (f * v + du)))
    return out


def _upd(res, stage, r, layer):
    if stage not in res or not r[0] <= res[stage][0]:
        res[stage] = (r[0], (layer,) + tuple(r[1]))


class _Acts:
    """The tensors of one parsed forward by their topology names."""

    def __init__(self, st, ctx):
        self.st, self.ctx = st, ctx

    def __call__(self, name):
        if name == "img":
            return self.ctx["image"]
        if name == "pool":
            return self.st["maxpool"].o[1]
        f = self.st["fwd"][name]
        return f["app"].o[7] if f["app"] is not None else self.st["mat"][name].o[7]

    def grad(self, src):
        kind, n = src
        if kind == "avgpool":
            return self.st["avgpool_bwd"].o[1]
        if kind == "maxpool":
            return self.st["maxpool_bwd"].o[2]
        b = self.st["bwd"][n]
        return b["dgrad"].o[3] if kind == "dx" else b["bn"].o[13]

    def upstream(self, name):
        """d = bf16(d1 + d2) of the topology's upstream gradients of ``name``, as bf16."""
        first, second = TOPO["grad"][name]
        d = self.grad(first)
        if second is not None:
            d2 = self.grad(second)
            if d is None or d2 is None:
                return None
            d = (d.float() + d2.float()).to(BF)
        return d


def check_forward_backward(st, ctx, res=None, only=None):
    """{stage: (largest error / bound over every element and every conv, (layer, index))} of one
    parsed forward + backward of the materialised chain.  ``ctx``: params {name: fp32 master
    before the step}, image (NHWC4 bf16), labels, label_smoothing, nbt (batches tracked before),
    prior {parameter: gradient the step adds onto} or None.  ``only``: a set of layer names
    ("head", "pool" and conv names) to restrict the work to."""
    res = {} if res is None else res
    act = _Acts(st, ctx)
    Pm, prior = ctx["params"], ctx.get("prior") or {}
    want = lambda n: only is None or n in only  # noqa: E731
    for c in TOPO["convs"]:
        n = c["name"]
        if not want(n):
            continue
        f, b = st["fwd"][n], st["bwd"][n]
        stem = c["role"] == "stem"
        wk = f["conv"].a[1]
        wb = bf(Pm[n + ".weight"])
        if stem:
            r = bitwise(wk[..., :3].contiguous(), wb)
            if wk.shape[-1] != 4 or bool((wk[..., 3] != 0).any()):
                r = (INF, ("channel 3",))
            _upd(res, "pad4", r, n)
            x = act("img")[..., :3]
        else:
            _upd(res, "weight_bf16", bitwise(wk, wb), n)
            x = act(c["src"])
        # ---- forward
        y = f["conv"].o[3]
        ref, A = conv_fwd(x, wb, c["s"], c["p"]), conv_fwd(x.abs(), wb.abs(), c["s"], c["p"])
        nacc = c["k"] * c["k"] * c["cin"]
        _upd(res, "conv_y", worst(y, ref, 2.0 ** -8 * ref.abs() + 2 * nacc * U * A + 1e-30), n)
        yd = f64(y).reshape(-1, c["cout"])
        P = yd.shape[0]
        s = f64(f["conv"].o[9])
        rs = max(worst(s[:, 0].sum(0), yd.sum(0), 2 * P * U * yd.abs().sum(0) + 1e-30),
                 worst(s[:, 1].sum(0), (yd * yd).sum(0), 2 * P * U * (yd * yd).sum(0) + 1e-30),
                 bitwise(f["fin"].a[0], f["conv"].o[9]), key=lambda t: t[0])
        if not bool(torch.isfinite(s).all()):
            rs = (INF, ("unwritten slab row",))
        _upd(res, "stats", rs, n)
        fb = bn_finalize_bounds(f["fin"].a[0], P, BN_EPS, BN_MOM, f["fin"].a[6], f["fin"].a[7])
        for k, i in (("mean", 8), ("invstd", 9), ("running_mean", 6), ("running_var", 7)):
            _upd(res, k, worst(f["fin"].o[i], *fb[k]), c["bn"])
        nb0, nb1 = int(f["fin"].a[10]), int(f["fin"].o[10])
        _upd(res, "nbt", (0.0, ()) if (nb0 == ctx["nbt"] and nb1 == ctx["nbt"] + 1) else (INF, (nb0, nb1)), c["bn"])
        mean, invstd = f["fin"].o[8], f["fin"].o[9]
        gamma, beta = Pm[c["bn"] + ".weight"], Pm[c["bn"] + ".bias"]
        out = act(n)
        rt = act(c["res"]) if c["res"] else None
        ref = R.bn_apply64(y, mean, invstd, gamma, beta, rt, c["relu"])
        sc = f64(invstd) * f64(gamma)
        mag = (f64(y) * sc).abs() + (f64(mean) * sc).abs() + f64(beta).abs() + (f64(rt).abs() if rt is not None else 0.0)
        _upd(res, "bn_apply", worst(out, ref, 2.0 ** -8 * ref.abs() + 4 * U * mag), c["bn"])
        # ---- BatchNorm backward
        d = act.upstream(n)
        if d is None or tuple(d.shape) != tuple(y.shape):
            _upd(res, "bn_bwd_dres", (INF, ("no upstream gradient of that shape",)), c["bn"])
            continue
        if c["relu"]:
            d = torch.where(f64(out) > 0, d, torch.zeros_like(d))
        if c["res"]:
            _upd(res, "bn_bwd_dres", bitwise(b["bn"].o[13], d), c["bn"])
        d = f64(d)
        rb = R.bn_bwd64(d, y, mean, invstd, gamma, float(P))
        E_d, E_q = 2 * P * U * rb["abs_d"], 2 * (P + 3) * U * rb["abs_dxh"]
        pg, pb = prior.get(c["bn"] + ".weight"), prior.get(c["bn"] + ".bias")
        if pg is None:
            _upd(res, "bn_dgamma", worst(b["bn"].o[9], rb["sum_dxh"], E_q), c["bn"])
            _upd(res, "bn_dbeta", worst(b["bn"].o[10], rb["sum_d"], E_d), c["bn"])
        else:
            pg, pb = f64(pg), f64(pb)
            _upd(res, "bn_dgamma", worst(b["bn"].o[9], pg + rb["sum_dxh"], 2 * (P + 4) * U * (rb["abs_dxh"] + pg.abs())), c["bn"])
            _upd(res, "bn_dbeta", worst(b["bn"].o[10], pb + rb["sum_d"], 2 * (P + 1) * U * (rb["abs_d"] + pb.abs())), c["bn"])
        kk = (f64(gamma) * f64(invstd) / P).abs()
        xh = rb["xh"].abs()
        bound = 2.0 ** -8 * rb["dx"].abs() + kk * (
            6 * U * (P * d.abs() + rb["sum_d"].abs() + xh * rb["sum_dxh"].abs()) + E_d + xh * E_q)
        dy = b["bn"].o[12]
        _upd(res, "bn_bwd_dy", worst(dy, rb["dx"], bound), c["bn"])
        # ---- data and weight gradients, from the stored dy
        if b["dgrad"] is not None:
            ref = conv_dgrad(x.shape, wb, dy, c["s"], c["p"])
            A = conv_dgrad(x.shape, wb.abs(), dy.abs(), c["s"], c["p"])
            nd = c["k"] * c["k"] * c["cout"]
            _upd(res, "dgrad", worst(b["dgrad"].o[3], ref, 2.0 ** -8 * ref.abs() + 2 * nd * U * A + 1e-30), n)
        wshape = tuple(wb.shape)
        pw = prior.get(n + ".weight")
        pw = None if pw is None else f64(pw)
        if b["red"] is None:
            ref, A = conv_wgrad(x, wshape, dy, c["s"], c["p"]), conv_wgrad(x.abs(), wshape, dy.abs(), c["s"], c["p"])
            nt = P
            if pw is not None:
                ref, A, nt = ref + pw, A + pw.abs(), P + 1
            _upd(res, "wgrad", worst(b["wgrad"].o[2].reshape(wshape), ref, 2 * nt * U * A + 1e-30), n)
        else:
            slab, ppc = b["wgrad"].o[2], int(b["wgrad"].a[7])
            ch = slab.shape[0]
            if ch != -(-P // ppc):
                _upd(res, "wgrad_slab", (INF, ("chunks", ch, P, ppc)), n)
                continue
            for r in range(ch):
                dr = chunk_of(f64(dy), r, ppc)
                ref, A = conv_wgrad(x, wshape, dr, c["s"], c["p"]), conv_wgrad(x.abs(), wshape, dr.abs(), c["s"], c["p"])
                rr = worst(slab[r].reshape(wshape), ref, 2 * ppc * U * A + 1e-30)
                _upd(res, "wgrad_slab", (rr[0], (r,) + rr[1]), n)
            s64 = f64(slab)
            ref = s64.sum(0) + (pw.reshape(-1) if pw is not None else 0.0)
            bound = K.reduce_bound(s64, 1.0, pw.reshape(-1) if pw is not None else None)
            _upd(res, "wgrad", worst(_dw_out(b).reshape(-1), ref, bound + 1e-30), n)
    if want("pool"):
        y_ref, idx, bwd = R.maxpool64(act("conv1"))
        r = bitwise(st["maxpool"].o[1], y_ref.to(BF))
        am = st["maxpool"].o[2].long()
        if tuple(am.shape) != tuple(idx.shape) or bool((am != idx).any()):
            r = (INF, ("argmax",))
        _upd(res, "maxpool", r, "maxpool")
        d = act.upstream("pool")
        wantd = bwd(d.float(), torch.float32).to(BF) if d is not None else None
        _upd(res, "maxpool_bwd", bitwise(st["maxpool_bwd"].o[2], wantd), "maxpool")
    if want("head"):
        last = act(TOPO["blocks"][-1]["name"] + ".conv2")
        N, H, W, Cc = last.shape
        A = f64(last).abs().reshape(N, H * W, Cc).sum(1)
        pooled = st["avgpool"].o[1]
        _upd(res, "avgpool", worst(pooled, R.avgpool64(last), 2 * (H * W + 1) * U * A / (H * W)), "avgpool")
        w, bias = f64(Pm["fc.weight"]), f64(Pm["fc.bias"])
        NC, Kd = w.shape
        xd = f64(pooled)
        gb = lambda k, mag: 2 * (2 * k + 3) * U * mag  # noqa: E731
        logits = st["head"].o[9]
        _upd(res, "head", worst(logits, xd @ w.t() + bias, gb(Kd, xd.abs() @ w.abs().t() + bias.abs())), "fc")
        B, eps = N, n32(ctx.get("label_smoothing", 0.0))
        g = n32(np.float32(1.0) / np.float32(B))
        lab = ctx["labels"]
        dl, loss = st["xent"].o[5], st["xent"].o[6]
        if eps:
            lref, dref, bl, bd = LS.bounds(logits, lab, eps, g)
        else:
            rows, p = R.xent_rows64(logits, lab)
            lref, dref = R.xent64(logits, lab, g)
            x = f64(logits)
            D = (x - x.max(1, keepdim=True).values).abs().max(1).values
            bd = g * (p * (2 * D[:, None] + 64) * U + 2 * U)
            lref, bl = lref.reshape(1), ((D + 64) * U * rows.abs().clamp(min=1.0)).mean().reshape(1)
        _upd(res, "loss", worst(loss.reshape(1), lref, bl), "loss")
        _upd(res, "dlogits", worst(dl, dref, bd), "loss")
        dd = f64(dl)
        hd, hw, hb = (c.o[9] for c in st["head_bwd"])
        _upd(res, "head_dx", worst(hd, dd @ w, gb(NC, dd.abs() @ w.abs())), "fc")
        pw, pb = prior.get("fc.weight"), prior.get("fc.bias")
        pw, pb = (f64(pw) if pw is not None else 0.0), (f64(pb) if pb is not None else 0.0)
        _upd(res, "head_dw", worst(hw, dd.t() @ xd + pw, gb(B, dd.abs().t() @ xd.abs() + abs(pw))), "fc")
        _upd(res, "head_db", worst(hb, dd.sum(0) + pb, gb(B, dd.abs().sum(0) + abs(pb))), "fc")
        ref = R.avgpool_bwd64(hd, H, W)
        _upd(res, "avgpool_bwd", worst(st["avgpool_bwd"].o[1], ref, (2.0 ** -8 + 2 * U) * ref.abs()), "avgpool")
    return res


def check_optimizer(sgd, st, ctx, res=None, landing_only=False):
    """Landing over the whole flat gradient buffer ``sgd`` read, then the update.  ``ctx``: layout
    {name: (offset, numel)}, grads_before (the flat buffer before the first backward, or None: zeros),
    hp (lr, momentum, weight_decay), first_step."""
    res = {} if res is None else res
    g = sgd.a[1]
    before = ctx.get("grads_before")
    inside = torch.zeros(g.numel(), dtype=torch.bool)
    worst_l = (0.0, ())
    prod = produced_grads(st)
    for n, (off, ne) in ctx["layout"].items():
        inside[off:off + ne] = True
        r = bitwise(g[off:off + ne], prod[n].reshape(-1))
        if r[0] > worst_l[0]:
            worst_l = (r[0], (n,) + r[1])
    gap_now = g[~inside]
    gap_was = before[~inside] if before is not None else torch.zeros_like(gap_now)
    r = bitwise(gap_now, gap_was)
    if r[0] > worst_l[0]:
        worst_l = (r[0], ("outside every view",) + r[1])
    res["landing"] = worst_l
    if landing_only:
        return res
    hp = ctx["hp"]
    a = dict(lr=n32(hp["lr"]), momentum=n32(hp["momentum"]), dampening=0.0, wd=n32(hp["weight_decay"]), nesterov=False)
    first = ctx["first_step"]
    p0, g64 = f64(sgd.a[0]), f64(g)
    m0 = torch.zeros_like(p0) if first else f64(sgd.a[2])
    pref, bref = R.sgd64(p0, g64, m0, first_step=first, **a)
    bp, bb = K.sgd_bounds(p0, g64, m0, first_step=first, **a)
    res["param"] = worst(sgd.o[0], pref, bp)
    res["momentum"] = worst(sgd.o[2], bref, bb)
    newb = bf(sgd.o[0])
    r16, r4 = (INF, ("no flat bf16 shadow",)), (INF, ("no PAD4 shadow",))
    for pre, post in zip(sgd.a[11], sgd.o[11]):
        off, ne, dst, kind = pre[0], pre[1], post[2], pre[3]
        if kind == K.SHADOW_BF16 and ne == newb.numel():
            r16 = bitwise(dst.reshape(-1), newb)
        elif kind == K.SHADOW_BF16_PAD4:
            d4 = dst.reshape(-1, 4)
            r4 = bitwise(d4[:, :3].contiguous().reshape(-1), newb[off:off + ne])
            if bool((d4[:, 3] != 0).any()):
                r4 = (INF, ("channel 3",))
            if (off, ne) != ctx["layout"]["conv1.weight"]:
                r4 = (INF, ("not the stem's slot", off, ne))
    res["shadow_bf16"], res["shadow_pad4"] = r16, r4
    return res


def check_step(trace, ctx, backwards=1, only=None, optimizer=True):
    """Parse and check one optimizer step of the materialised chain: ``backwards`` forward +
    backward passes (the last one is checked, with ``ctx["prior"]``), then the optimizer."""
    res = {}
    try:
        sts, sgd = parse_trace(trace, backwards)
    except OrderError as e:
        return {"order": (INF, (str(e),))}
    res["order"] = (0.0, ())
    check_forward_backward(sts[-1], ctx, res, only)
    if optimizer:
        check_optimizer(sgd, sts[-1], ctx, res, landing_only=only is not None)
    return res


# ------------------------------------------------------------------------------- emulation
def make_model(num_classes, seed=0):
    """{name: fp32 tensor}: parameters (conv weights OHWI, kaiming fan-out scale; gamma in
    [0.5, 1.5], beta ~ 0.1 N) and BatchNorm buffers (running_mean ~ 0.1 N, running_var in [0.5, 1.5])."""
    g = torch.Generator().manual_seed(3000 + seed)
    P, Bf = {}, {}
    for c in TOPO["convs"]:
        std = (2.0 / (c["k"] * c["k"] * c["cout"])) ** 0.5
        P[c["name"] + ".weight"] = torch.randn(c["cout"], c["k"], c["k"], c["cin"], generator=g) * std
        P[c["bn"] + ".weight"] = torch.rand(c["cout"], generator=g) + 0.5
        P[c["bn"] + ".bias"] = torch.randn(c["cout"], generator=g) * 0.1
        Bf[c["bn"] + ".running_mean"] = torch.randn(c["cout"], generator=g) * 0.1
        Bf[c["bn"] + ".running_var"] = torch.rand(c["cout"], generator=g) + 0.5
    bound = 1.0 / 512 ** 0.5
    P["fc.weight"] = (torch.rand(num_classes, 512, generator=g) * 2 - 1) * bound
    P["fc.bias"] = (torch.rand(num_classes, generator=g) * 2 - 1) * bound
    return P, Bf


def make_batch(B, size, num_classes, seed=0):
    """(NHWC4 bf16 image batch with channel 3 zero, int64 labels)."""
    g = torch.Generator().manual_seed(4000 + seed)
    img = torch.zeros(B, size, size, 4, dtype=BF)
    img[..., :3] = torch.randn(B, size, size, 3, generator=g).to(BF)
    return img, torch.randint(0, num_classes, (B,), generator=g)


def _args(n, **at):
    a = [None] * n
    for k, v in at.items():
        a[int(k[1:])] = v
    return a


def emulate_forward_backward(P, Bf, img, labels, grads, nbt, label_smoothing=0.0, overwrite=False, ppc_max=1024,
                             plant=None):
    """The calls of one forward + backward in float32 / bf16.  ``P`` masters, ``Bf`` BatchNorm
    buffers (updated in place), ``grads`` {name: tensor} (added onto, or overwritten with
    ``overwrite``; updated in place), ``nbt`` batches tracked so far.  ``plant``: see ``PLANTS``."""
    f32 = torch.float32
    T, acts, raw, fin_of = [], {"img": img}, {}, {}
    B = img.shape[0]

    def put(name, val):
        if overwrite or name not in grads:
            grads[name] = val.clone()
        else:
            grads[name] = grads[name] + val
        return grads[name].clone()

    for c in TOPO["convs"]:
        n, stem = c["name"], c["role"] == "stem"
        wb = bf(P[n + ".weight"])
        wk = F.pad(wb, (0, 1)) if stem else wb
        if stem and plant == "pad4_nonzero":
            wk = wk.clone()
            wk[5, 3, 3, 3] = 2.0 ** -10
        xin = acts[c["src"]]
        x = xin[..., :3] if stem else xin
        y = conv_fwd(x, wb, c["s"], c["p"], f32).to(BF)
        Pn = y.numel() // c["cout"]
        yf = y.float().reshape(Pn, -1)
        rows = -(-Pn // 128)
        stats = torch.zeros(rows, 2, c["cout"])
        for r in range(rows):
            blk = yf[r * 128:(r + 1) * 128]
            stats[r, 0], stats[r, 1] = blk.sum(0), (blk * blk).sum(0)
        T.append(Call("conv_gemm_fwd", _args(11, a0=xin, a1=wk), _args(11, a3=y, a9=stats)))
        cnt, mom = float(Pn), n32(BN_MOM)
        keep_w = float(np.float32(1.0) - np.float32(BN_MOM))
        mean = stats[:, 0].sum(0) / cnt
        var = (stats[:, 1].sum(0) / cnt - mean * mean).clamp(min=0.0)
        invstd = (var + n32(BN_EPS)).rsqrt()
        unb = var * cnt / (cnt - 1.0) if (Pn > 1 and plant != "biased_var") else var
        rm0, rv0 = Bf[c["bn"] + ".running_mean"], Bf[c["bn"] + ".running_var"]
        if plant == "momentum_swapped":
            rm1 = rm0 * mom + mean * keep_w
        else:
            rm1 = rm0 * keep_w + mean * mom
        rv1 = rv0 * keep_w + unb * mom
        nb1 = nbt if plant == "nbt_stuck" else nbt + 1
        T.append(Call("bn_finalize", _args(12, a0=stats, a6=rm0, a7=rv0, a10=torch.tensor(nbt)),
                      _args(12, a6=rm1, a7=rv1, a8=mean, a9=invstd, a10=torch.tensor(nb1))))
        Bf[c["bn"] + ".running_mean"], Bf[c["bn"] + ".running_var"] = rm1, rv1
        gamma, beta = P[c["bn"] + ".weight"], P[c["bn"] + ".bias"]
        sc = invstd * gamma
        v = y.float() * sc + (beta - mean * sc)
        pre = v
        res_name = c["res"]
        if res_name and plant == "res_from_conv1" and n == "layer1.1.conv2":
            res_name = "layer1.1.conv1"
        if res_name:
            v = v + acts[res_name].float()
        relu = c["relu"] or (plant == "relu_after_ds" and n == "layer2.0.downsample.0")
        out = (torch.relu(v) if relu else v).to(BF)
        T.append(Call("bn_apply", _args(8, a0=y), _args(8, a7=out)))
        acts[n], raw[n] = out, (y, mean, invstd, gamma, pre, xin)
        if stem:
            y_ref, idx, pool_bwd = R.maxpool64(out)
            acts["pool"] = y_ref.to(BF)
            T.append(Call("maxpool_fwd", _args(4, a0=out), _args(4, a1=acts["pool"], a2=idx.to(torch.uint8))))
    last = acts[TOPO["blocks"][-1]["name"] + ".conv2"]
    N, H, W, Cc = last.shape
    pooled = last.float().reshape(N, H * W, Cc).sum(1) / float(H * W)
    T.append(Call("avgpool_fwd", _args(2, a0=last), _args(2, a1=pooled)))
    logits = pooled @ P["fc.weight"].t() + P["fc.bias"]
    T.append(Call("sgemm", _args(13), _args(13, a9=logits)))
    lp = torch.log_softmax(logits, 1)
    eps, NC = n32(label_smoothing), logits.shape[1]
    onehot = F.one_hot(labels, NC).float()
    tgt = onehot * n32(1.0 - eps) + n32(eps / NC)
    loss = -(tgt * lp).sum(1).sum() / float(B)
    gs = 1.0 if plant == "no_1_over_B" else n32(np.float32(1.0) / np.float32(B))
    dl = (lp.exp() - tgt) * gs
    T.append(Call("xent", _args(10, a0=logits), _args(10, a5=dl, a6=loss.reshape(1))))
    hd = dl @ P["fc.weight"]
    T.append(Call("sgemm", _args(13), _args(13, a9=hd)))
    T.append(Call("sgemm", _args(13), _args(13, a9=put("fc.weight", dl.t() @ pooled))))
    T.append(Call("sgemm", _args(13), _args(13, a9=put("fc.bias", dl.sum(0)))))
    dpool = (hd / float(H * W))[:, None, None, :].expand(N, H, W, Cc).to(BF).contiguous()
    T.append(Call("avgpool_bwd", _args(2, a0=hd), _args(2, a1=dpool)))
    G = {("avgpool", None): dpool}

    def conv_bwd(n):
        c = CONV[n]
        y, mean, invstd, gamma, pre, xin = raw[n]
        first, second = TOPO["grad"][n]
        d = G[first].float()
        if second is not None and not (plant == "stash_dropped" and n == "layer1.0.conv2"):
            d2 = G[second].float()
            if plant == "stash_twice" and n == "layer1.0.conv2":
                d2 = d2 * 2
            d = (d + d2).to(BF).float()
        if c["relu"]:
            keep = (pre.to(BF) > 0) if (plant == "mask_pre_residual" and n == "layer1.1.conv2") else (acts[n] > 0)
            d = torch.where(keep, d, torch.zeros_like(d))
        Pn = float(y.numel() // c["cout"])
        xh = (y.float() - mean) * invstd
        sd, sq = d.reshape(-1, c["cout"]).sum(0), (d * xh).reshape(-1, c["cout"]).sum(0)
        dy = ((gamma * invstd / Pn) * (Pn * d - sd - xh * sq)).to(BF)
        if plant == "dgamma_dbeta_swapped" and n == "layer2.1.conv1":
            sd, sq = sq, sd
        og, ob = put(c["bn"] + ".weight", sq), put(c["bn"] + ".bias", sd)
        dres = d.to(BF) if c["res"] else None
        T.append(Call("bn_bwd", _args(16), _args(16, a9=og, a10=ob, a12=dy, a13=dres)))
        G[("dres", n)] = dres
        wb = bf(P[n + ".weight"])
        stem = c["role"] == "stem"
        x = xin[..., :3] if stem else xin
        if not stem:
            dx = conv_dgrad(x.shape, wb, dy, c["s"], c["p"], f32).to(BF)
            T.append(Call("conv_gemm_dgrad", _args(9), _args(9, a3=dx)))
            G[("dx", n)] = dx
        Pi = int(Pn)
        ppc = min(ppc_max, -(-Pi // 32) * 32)
        ch = -(-Pi // ppc)
        if ch == 1:
            dw = put(n + ".weight", conv_wgrad(x, wb.shape, dy, c["s"], c["p"], f32))
            T.append(Call("conv_gemm_wgrad", _args(11, a2=torch.empty(wb.shape), a7=ppc), _args(11, a2=dw)))
        else:
            slab = torch.stack([conv_wgrad(x, wb.shape, chunk_of(dy.float(), r, ppc), c["s"], c["p"], f32).reshape(-1)
                                for r in range(ch)])
            T.append(Call("conv_gemm_wgrad", _args(11, a2=torch.empty_like(slab), a7=ppc), _args(11, a2=slab)))
            dw = put(n + ".weight", slab.sum(0).view(wb.shape))
            T.append(Call("grad_reduce", [[(slab,)]], [[(slab, 0, 0, 0, ch, dw.reshape(-1))]]))

    for b in reversed(TOPO["blocks"]):
        for role in ("conv2", "downsample.0", "conv1"):
            if b["name"] + "." + role in CONV:
                conv_bwd(b["name"] + "." + role)
    first, second = TOPO["grad"]["pool"]
    d = (G[first].float() + G[second].float()).to(BF)
    G[("maxpool", None)] = pool_bwd(d.float(), torch.float32).to(BF)
    T.append(Call("maxpool_bwd", _args(4), _args(4, a2=G[("maxpool", None)])))
    conv_bwd("conv1")
    return T


def emulate_sgd(P, grads, mom, hp, first, grads_before=None, plant=None):
    """The optimizer call over this file's own flat layout; returns (Call, layout, new masters,
    new momentum {name: tensor})."""
    shapes = {k: tuple(v.shape) for k, v in P.items()}
    lay, total = flat_layout(shapes)
    p = torch.zeros(total)
    g = torch.zeros(total) if grads_before is None else grads_before.clone()
    m = torch.zeros(total)
    src = dict(grads)
    if plant == "wgrad_wrong_slot":
        src["layer1.0.conv1.weight"] = grads["layer1.0.conv2.weight"]
    for n, (off, ne) in lay.items():
        p[off:off + ne] = P[n].reshape(-1)
        g[off:off + ne] = src[n].reshape(-1)
        if mom is not None:
            m[off:off + ne] = mom[n].reshape(-1)
    d = g + p * n32(hp["weight_decay"])
    buf = d.clone() if first else m * n32(hp["momentum"]) + d
    pn = p - buf * n32(hp["lr"])
    off, ne = lay["conv1.weight"]
    pad4 = F.pad(pn[off:off + ne].to(BF).view(-1, 3), (0, 1))
    sh_pre = [(0, total, None, K.SHADOW_BF16, 0, 0, 0), (off, ne, None, K.SHADOW_BF16_PAD4, 0, 0, 0)]
    sh_post = [(0, total, pn.to(BF), K.SHADOW_BF16, 0, 0, 0), (off, ne, pad4, K.SHADOW_BF16_PAD4, 0, 0, 0)]
    call = Call("sgd", _args(12, a0=p, a1=g, a2=m, a11=sh_pre), _args(12, a0=pn, a2=buf, a11=sh_post))
    newP = {n: pn[o:o + k].view(shapes[n]).clone() for n, (o, k) in lay.items()}
    newM = {n: buf[o:o + k].view(shapes[n]).clone() for n, (o, k) in lay.items()}
    return call, lay, newP, newM


PLANTS = ("res_from_conv1", "stash_dropped", "stash_twice", "relu_after_ds", "biased_var", "momentum_swapped",
          "dgamma_dbeta_swapped", "wgrad_wrong_slot", "accumulate_second_step", "no_1_over_B", "mask_pre_residual",
          "pad4_nonzero", "nbt_stuck")
CASES = {"s64": dict(size=64, B=4, classes=10, label_smoothing=0.0, steps=2),
         "s72": dict(size=72, B=3, classes=1000, label_smoothing=0.1, steps=1),
         "accum": dict(size=64, B=2, classes=10, label_smoothing=0.0, steps=1, micro=2)}
HP = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
