"""One SimpleCNN training step on the module path, stage by stage and element by element, against
float64: ops/functional.py's four autograd Functions, SimpleCNN.forward, the FlatSpace gradient
views autograd accumulates into and FusedSGD (tests/test_simplecnn_step_elementwise_gpu.py records
the step on the GPU and runs it through ``check_step``; tests/test_simplecnn_step_bounds_cpu.py
shows that ``check_step`` admits a correct step and rejects wrong ones).  A helper module, not a
test module; it needs no GPU.

Recording.  ``resnet_step_cases.Recorder`` with this file's ``KERNELS`` and ``OUTPUTS``: the
Functions allocate their outputs with torch.empty, so the proxy fills every output argument of a
call with NaN before the launch and an element the kernel leaves unwritten is a NaN in the trace
(``worst`` counts it as infinitely far out).  Sentinel bands around those buffers are not possible
here; they stay with tests/test_simplecnn_kernels_elementwise_gpu.py.  What no kernel call shows
- the gradient a Function returns for fl.bias (``go.sum(0)``), what AccumulateGrad makes of the
returned gradients - the GPU test takes from tensor hooks on the parameters (``hooked``) and from
copies of the flat gradient buffer before and after every backward.

A step record: ``trace`` (the Calls of the step, in order), ``params`` {name: master before the
step}, ``momentum_before`` (flat, None on the first step), ``first_step``, ``dtype``, ``layout`` /
``total`` (the FlatSpace's), ``hp`` and ``micro``: per forward + backward ``x`` [B,1,28,28] float
(what the model was given), ``u8`` (the uint8 images behind it, loader cases), ``labels``,
``scale`` (the factor the loss is multiplied with before backward), ``eps`` (label smoothing),
``hooked`` {name: gradient the Function returned}, ``grads_before`` / ``grads_after`` (the flat
gradient buffer around the backward) and ``gx`` (x.grad, the input_grad case).

Checking.  ``check_step`` is teacher-forced: the float64 reference of a stage is computed from
exactly the tensors that call read, as recorded, so errors do not compound and every bound is
the one-kernel bound; that the call read the RIGHT tensors is the business of the ``wire_*``
stages, which compare operands bit for bit with the stored output of the stage that should feed
them and scalar arguments with their values.  Masks come from the stored activations: no ReLU
ambiguity, no element exempt.  Nothing is calibrated on the kernels.

Stages, in dependency order (u = 2**-24, n = accumulated terms, A = the operation on absolute
values, E = 2 n u A, 3 n u A for the fp32 cases where the stage's products round too, a bf16
output 2**-8 (|ref| + E) + E - ddp_amd/ops/kernel_bounds.py; the n are those of
tests/test_simplecnn_kernels_elementwise_gpu.py).  Every E, dl_scaled and landing also carry n 2**-126,
one smallest normal fp32 per operation: a real step's gradients reach below it (a dW element of
3e-46 is stored as 0), where an fp32 operation errs by up to 2**-150 with gradual underflow and by
up to 2**-126 where the hardware flushes to zero, whatever u says:

  order        per forward + backward exactly conv1_fwd, conv3x3_fwd, fc_partial, fc_reduce, xent,
               fc_bwd, conv3x3_dgrad, conv3x3_wgrad, grad_reduce, conv1_wgrad, grad_reduce; one
               sgd after the last; nothing else
  layout       the FlatSpace's {name: (offset, numel)} and length equal ``flat_layout`` of the
               shapes (reverse registration order, 64-element alignment)
  zeroed       before a step's first backward the whole flat gradient buffer is zero.  SimpleCNN's
               module path takes no lazy zero: its Functions return their gradients and autograd's
               AccumulateGrad adds them into the views, no direct_grad producer writes them, so
               FusedSGD.zero_grad always memsets (direct_grad.lazy_zero is False) and there is
               nothing to pre-fill with NaN - a NaN would be added to, not overwritten
  wire_conv1   x: bit for bit the float input (loader cases: within 2 u (1 + u) |u8 / 255| - torch
               divides by a scalar as a multiplication with fl(1 / 255), two roundings); w, b the
               masters; no index list; B, H, W
  a1           conv1_fwd, n = 10
  wire_conv2   x = the stored a1, w = w2.to(dtype) of the step's masters, b = b2, ReLU, no fused fc, pxt 2
  a2           conv3x3_fwd, n = 9 * 32 + 1
  wire_fc      fc_partial reads the stored a2 and wfc.to(dtype) ([out][HW][C] as the master holds
               it); fc_reduce the stored partials, bfc, (B, 49, 10)
  fc_partial   n = 16 * 64 + 6
  fc_reduce    n = 49 + 1, from the partials it read
  wire_xent    the stored logits, G = 1, no bias, the labels, gscale = 1 / B of THIS batch,
               label_smoothing by keyword exactly when it is not 0
  dlogits,     no smoothing: g (p (2 D + 64) u + 2 u) and mean (D + 64) u max(1, |row|) (with G = 1
  loss         and no bias the kernel's logit is the stored one exactly); smoothing:
               label_smoothing_cases.bounds.  g = fl32(1 / B)
  dl_scaled    fc_bwd's dL = dl * scale: one rounding, u |ref|
  wire_fc_bwd  X = the stored a2 (the saved tensor), W = the forward's operand, scale 1.0, mask
               False (the ReLU mask of dX is applied by conv2's backward kernels, from a2), dX
               and dW given, no dbias / loss arguments
  fc_dx        n = NO (unmasked);  fc_dw  n = B + 2
  fc_db        the hooked fl.bias gradient against sum_b dL: n = B
  wire_dgrad   dy = the stored dX, mask = the stored a2, weight = bit for bit the [tap][ci][co]
               permutation of w2.to(dtype) of the step's masters, no x mask, pxt 2
  dz1          conv3x3_dgrad, n = 9 * 64, dy masked by a2 > 0.  The module path passes no a1 mask
               here (conv1_wgrad applies it), so no output element is forced to 0 by a mask of its
               own; where every contributing dy is masked A = 0 and the element must be exactly 0
  wire_wgrad   dy = the stored dX, mask = the stored a2, x = the stored a1 (the saved xb), R =
               functional.wgrad_rows(28, B, dtype), slab [B ceil(28 / R)][64 * 9 * 32 + 64] fp32
  w2slab       every slab row, n = wgrad_nslot(28, R)
  wire_red2    two segments over the wgrad's slab: (row, 0, 18432, rows, scale 1) and (row, 18432,
               64, rows, scale 1), no accumulate flag
  gw2, gb2     against the float64 sum of the rows' references: the rows' bounds summed plus
               2 (rows + 2) u sum|row| of the stored rows
  replay_w2,   bit for bit kernel_bounds.replay_reduce of the stored rows, groups =
  replay_b2    kernel_bounds.reduce_groups
  wire_conv1w  x = the forward's xf (the saved tensor), dy = the stored dZ1, mask = the stored a1,
               (B, 28, 28, 32, chunk 256), slab [ceil(B 784 / 256)][320] fp32
  w1slab       every slab row, n = chunk = 256
  wire_red1, gw1, gb1, replay_w1, replay_b1: as conv2's, rows of 320 = 288 + 32
  returned     the hooked gradients of the four conv parameters and fl.weight are bit for bit the
               reducers' / fc_bwd's outputs
  landing      every view of the flat gradient buffer after the backward against prior + returned
               gradient in float64: one rounding, u |sum|
  gaps         the alignment gaps of the flat gradient buffer are exactly 0 after the backward
  input_grad   (input_grad case) x.grad of _Conv1ReLU.backward's conv_transpose2d fallback
               against float64: norm-relative 1e-5, the figure tests/test_fp32_gpu.py uses for fp32
               paths - not an a-priori bound, the library chooses the algorithm
  wire_sgd     parameters = the masters, gradients = the buffer after the last backward, momentum
               = the previous step's (zeros on the first), lr / momentum / dampening / weight
               decay / flags, first_step only on the first step, update True, no clip, no schedule
  param,       kernel_bounds.sgd_bounds over the whole flat buffers
  momentum
  state_gaps   the gaps of the parameter and momentum buffers are exactly 0 after sgd

``emulate_case`` is a plain fp32 / bf16 model of the cases (torch's float32 operators, bf16
roundings at the kernels' store points, the reducer's order from kernel_bounds.replay_reduce)
that emits step records; ``plant=`` plants one wiring error (``PLANTS``).
"""
import functools
import math

import numpy as np
import torch

import elementwise as EW
import label_smoothing_cases as LS
from ddp_amd.ops import kernel_bounds as K
from ddp_amd.ops import reference as R
from ddp_amd.ops.functional import wgrad_rows
from ddp_amd.ops.kernel_bounds import bf16_store_bound
from elementwise import BF, F32, INF, U, bits, bitwise, f64, n32, worst  # noqa: F401  (reachable as S.worst ...)
from engine_step_cases import w1_rows_of, wgrad_nslot, wgrad_rows_of
from resnet_step_cases import Call, OrderError, Recorder, _Cursor  # noqa: F401

H = W = 28
HW, C1, C2, NO, CHUNK, ALIGN = H * W, 32, 64, 10, 256, 64
TINY = 2.0 ** -126  # the smallest normal fp32
NW2, ROW2, NW1, ROW1 = C2 * 9 * C1, C2 * 9 * C1 + C2, C1 * 9, C1 * 10
NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "fl.weight", "fl.bias")  # registration order
SHAPES = {"net.0.weight": (C1, 3, 3, 1), "net.0.bias": (C1,), "net.2.weight": (C2, 3, 3, C1), "net.2.bias": (C2,),
          "fl.weight": (NO, HW, C2), "fl.bias": (NO,)}
HP = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
FWD_BWD = (("c1", "conv1_fwd", "conv1 forward"), ("c2", "conv3x3_fwd", "conv2 forward"), ("fcp", "fc_partial", "fc partials"),
           ("fcr", "fc_reduce", "fc reduction"), ("xe", "xent", "loss"), ("fcb", "fc_bwd", "fc backward"),
           ("dg", "conv3x3_dgrad", "conv2 data gradient"), ("wg", "conv3x3_wgrad", "conv2 weight gradient"),
           ("red2", "grad_reduce", "conv2 slab reduction"), ("c1w", "conv1_wgrad", "conv1 weight gradient"),
           ("red1", "grad_reduce", "conv1 slab reduction"))
KERNELS = {name for _, name, _ in FWD_BWD} | {"sgd"}
# the arguments each call must write in full (NaN-filled before the launch)
OUTPUTS = {"conv1_fwd": lambda a, kw: [a[7]], "conv3x3_fwd": lambda a, kw: [a[3]], "fc_partial": lambda a, kw: [a[2]],
           "fc_reduce": lambda a, kw: [a[2]], "xent": lambda a, kw: [a[5], a[6]], "fc_bwd": lambda a, kw: [a[3], a[4]],
           "conv3x3_dgrad": lambda a, kw: [a[4]], "conv3x3_wgrad": lambda a, kw: [a[3]],
           "conv1_wgrad": lambda a, kw: [a[7]], "grad_reduce": lambda a, kw: [s[5] for s in a[0]]}
STAGES = ("order", "layout", "zeroed", "wire_conv1", "a1", "wire_conv2", "a2", "wire_fc", "fc_partial", "fc_reduce",
          "wire_xent", "dlogits", "loss", "dl_scaled", "wire_fc_bwd", "fc_dx", "fc_dw", "fc_db", "wire_dgrad", "dz1",
          "wire_wgrad", "w2slab", "wire_red2", "gw2", "gb2", "replay_w2", "replay_b2", "wire_conv1w", "w1slab",
          "wire_red1", "gw1", "gb1", "replay_w1", "replay_b1", "returned", "landing", "gaps", "input_grad", "wire_sgd",
          "param", "momentum", "state_gaps")
failing = functools.partial(EW.failing, order=STAGES)                            # failing(res)
report = functools.partial(EW.report, order=STAGES, tag="SIMPLECNN_STEP_RATIO")  # report(res, case)


def _case(dtype, steps, eps=0.0, accum=1, loader=False, input_grad=False):
    return dict(dtype=dtype, steps=steps, eps=eps, accum=accum, loader=loader, input_grad=input_grad)


# steps: per optimizer step the batch sizes of its forward + backward passes.  B = 1, 10, 19, 32 are
# the smallest batches that reach wgrad_rows' branches R = 1, 2, 4, 7 (fp32: 1, 2, 4)
CASES = {"b1_bf16": _case(BF, [[1]]), "b1_fp32": _case(F32, [[1]]), "b3": _case(BF, [[3], [3]]),
         "b10_bf16": _case(BF, [[10]]), "b10_fp32": _case(F32, [[10]]), "b19_bf16": _case(BF, [[19]]),
         "b19_fp32": _case(F32, [[19]]), "b32": _case(BF, [[32]]), "ragged": _case(BF, [[10], [7]], loader=True),
         "smooth": _case(BF, [[3]], eps=0.1), "accum": _case(BF, [[3, 3]], accum=2),
         "input_grad": _case(F32, [[1]], input_grad=True)}
WGRAD_ROWS = {(BF, 1): 1, (BF, 10): 2, (BF, 19): 4, (BF, 32): 7, (F32, 1): 1, (F32, 10): 2, (F32, 19): 4}


# ------------------------------------------------------------------------------- layout, inputs
def flat_layout(shapes=SHAPES, align=ALIGN):
    """{name: (offset, numel)} and the buffer's length: reverse registration order, every
    parameter on an ``align``-element boundary."""
    off, lay = 0, {}
    for n in reversed(NAMES):
        ne = math.prod(shapes[n])
        lay[n] = (off, ne)
        off += (ne + align - 1) // align * align
    return lay, off


def inside_mask(layout, total):
    m = torch.zeros(total, dtype=torch.bool)
    for off, ne in layout.values():
        m[off:off + ne] = True
    return m


def to_flat(named, layout, total):
    out = torch.zeros(total)
    for n, (off, ne) in layout.items():
        out[off:off + ne] = named[n].reshape(-1)
    return out


def masters(seed=0):
    """{name: fp32 master} in the native layouts (OHWI conv weights, [out][HW][C] fc weight)."""
    g = torch.Generator().manual_seed(5000 + seed)
    scale = {"net.0.weight": 0.3, "net.0.bias": 0.1, "net.2.weight": 0.08, "net.2.bias": 0.05, "fl.weight": 0.006,
             "fl.bias": 0.05}
    return {n: torch.randn(*SHAPES[n], generator=g) * scale[n] for n in NAMES}


def case_inputs(case):
    """Per optimizer step, per forward + backward: (x [B,1,28,28] float or None, u8 [B,28,28] or
    None, labels int64 [B]).  Loader cases return the 17-image dataset in ``u8`` of the first entry
    instead (see ``loader_dataset``): the loader chooses the images."""
    cs = CASES[case]
    g = torch.Generator().manual_seed(6000 + sum(map(sum, cs["steps"])))
    out = []
    for sizes in cs["steps"]:
        out.append([(torch.rand(B, 1, H, W, generator=g), None, torch.randint(0, NO, (B,), generator=g)) for B in sizes])
    return out


def loader_dataset(n=17):
    g = torch.Generator().manual_seed(6100)
    return torch.randint(0, 256, (n, H, W), generator=g, dtype=torch.uint8), torch.randint(0, NO, (n,), generator=g)


# ------------------------------------------------------------------------------- parsing
def parse_trace(trace, backwards):
    """[{key: Call} per forward + backward], the sgd Call."""
    cur = _Cursor(trace)
    sts = [{key: cur.take(name, f"{layer} (pass {k})") for key, name, layer in FWD_BWD} for k in range(backwards)]
    sgd = cur.take("sgd", "optimizer")
    if cur.peek() is not None:
        raise OrderError(f"after the optimizer: {len(trace) - cur.i} extra calls, first {cur.peek()}")
    return sts, sgd


# ------------------------------------------------------------------------------- checking
def _upd(res, stage, r, what=""):
    if stage not in res or not r[0] <= res[stage][0]:
        res[stage] = (r[0], (what,) + tuple(r[1]))


def _same(res, stage, what, got, want):
    """A scalar / structural argument: equal or infinitely far out."""
    try:
        ok = bool(got == want)
    except (RuntimeError, TypeError, ValueError):  # a tensor where a scalar belongs
        ok = False
    _upd(res, stage, (0.0, ()) if ok else (INF, (repr(got)[:200], repr(want)[:200])), what)


def _bit(res, stage, what, got, want):
    _upd(res, stage, bitwise(got, want), what)


def acc_bound(n, A, f32_operands=False):
    """kernel_bounds.acc_bound plus the underflow term of the module docstring."""
    return K.acc_bound(n, A, f32_operands) + n * TINY


def _out(ref, E, dtype):
    return bf16_store_bound(ref, E) if dtype == BF else E


def _seg_check(res, stage, red, slab_call_out, row, nw, nb, rows):
    segs = red.a[0]
    _same(res, stage, "segments", len(segs), 2)
    for k, (off, n) in enumerate(((0, nw), (nw, nb))[:len(segs)]):
        s = segs[k]
        _bit(res, stage, f"segment {k} slab", s[0], slab_call_out)
        _same(res, stage, f"segment {k} (stride, offset, n, rows)", tuple(s[1:5]), (row, off, n, rows))
        _same(res, stage, f"segment {k} scale", float(s[6]), 1.0)
        _same(res, stage, f"segment {k} accumulate", bool(len(s) > 7 and s[7]), False)


def _reduced(res, names, red, slab, ref_rows, E_rows, nw):
    """gw / gb against the rows' references, and the order replay, from the slab the reducer read."""
    s64 = f64(slab)
    if tuple(s64.shape) != tuple(ref_rows.shape) or len(red.o[0]) != 2:
        for n in names:
            _upd(res, n, (INF, ("slab shape / segments",)))
        return
    tot = E_rows.sum(0) + K.reduce_bound(s64, 1.0)
    rows32 = slab.numpy()
    GR = K.reduce_groups([rows32.shape[0]] * 2)
    for (stage, replay), sl in zip((names[:2], names[2:]), (slice(0, nw), slice(nw, None))):
        out = red.o[0][0 if sl.start == 0 else 1][5]
        _upd(res, stage, worst(out.reshape(-1), ref_rows[:, sl].sum(0), tot[sl]))
        _upd(res, replay, bitwise(out.reshape(-1), torch.from_numpy(K.replay_reduce(rows32[:, sl], GR))))


def check_pass(st, m, rec, res, first_of_step):
    """One parsed forward + backward ``st`` with its record ``m`` into ``res``."""
    dt, P = rec["dtype"], rec["params"]
    f32b = dt == F32
    B = m["labels"].shape[0]
    lay, total = rec["layout"], rec["total"]
    c1, c2, fcp, fcr, xe, fcb, dg, wg, red2, c1w, red1 = (st[k] for k, _, _ in FWD_BWD)
    if first_of_step:
        _upd(res, "zeroed", (0.0, ()) if not bool((m["grads_before"] != 0).any()) else (INF, ("gradient buffer not zero",)))
    # ---- conv1 forward
    xf = c1.a[0]
    if m.get("u8") is not None:
        ref = (f64(m["u8"]) / 255.0).reshape(B, HW)
        _upd(res, "wire_conv1", worst(xf, ref, 2 * U * (1 + U) * ref.abs()), "x = u8 / 255")
    else:
        _bit(res, "wire_conv1", "x", xf, m["x"].reshape(B, HW))
    _bit(res, "wire_conv1", "w", c1.a[5], P["net.0.weight"])
    _bit(res, "wire_conv1", "b", c1.a[6], P["net.0.bias"])
    _same(res, "wire_conv1", "index list / offsets", tuple(c1.a[1:5]), (None, None, 0, 0))
    _same(res, "wire_conv1", "(B, H, W)", tuple(c1.a[8:11]), (B, H, W))
    a1 = c1.o[7]
    _same(res, "wire_conv1", "output dtype", a1.dtype, dt)
    x3 = f64(xf).reshape(B, H, W)
    ref = R.conv1_64(x3, f64(c1.a[5]).reshape(C1, 9), c1.a[6])
    A = R.conv3x3_64(x3.abs().unsqueeze(-1), f64(c1.a[5]).abs().reshape(C1, 3, 3, 1), f64(c1.a[6]).abs())
    _upd(res, "a1", worst(a1, ref, _out(ref, acc_bound(10, A), dt)))
    # ---- conv2 forward
    _bit(res, "wire_conv2", "x = stored a1", c2.a[0], a1)
    _bit(res, "wire_conv2", "w = w2.to(dtype) of the masters", c2.a[1], P["net.2.weight"].to(dt))
    _bit(res, "wire_conv2", "b", c2.a[2], P["net.2.bias"])
    _same(res, "wire_conv2", "(relu, fc weight, fc partials, NO, pxt)", tuple(c2.a[4:9]), (True, None, None, 0, 2))
    a2 = c2.o[3]
    ref = R.conv3x3_64(c2.a[0], c2.a[1], c2.a[2], True)
    A = R.conv3x3_64(f64(c2.a[0]).abs(), f64(c2.a[1]).abs(), f64(c2.a[2]).abs())
    _upd(res, "a2", worst(a2, ref, _out(ref, acc_bound(9 * C1 + 1, A, f32b), dt)))
    # ---- fc
    _bit(res, "wire_fc", "x = stored a2", fcp.a[0], a2)
    _bit(res, "wire_fc", "w = wfc.to(dtype) of the masters", fcp.a[1], P["fl.weight"].to(dt))
    _bit(res, "wire_fc", "fc_reduce partials", fcr.a[0], fcp.o[2])
    _bit(res, "wire_fc", "bias", fcr.a[1], P["fl.bias"])
    _same(res, "wire_fc", "(B, G, NO)", tuple(fcr.a[3:6]), (B, HW // 16, NO))
    xt, wt = f64(fcp.a[0]).reshape(B, HW // 16, 16 * C2), f64(fcp.a[1]).reshape(NO, HW // 16, 16 * C2)
    pref, pA = torch.einsum("bgk,ogk->bgo", xt, wt), torch.einsum("bgk,ogk->bgo", xt.abs(), wt.abs())
    _upd(res, "fc_partial", worst(fcp.o[2], pref, acc_bound(16 * C2 + 6, pA, f32b)))
    p64 = f64(fcr.a[0])
    logits = fcr.o[2]
    _upd(res, "fc_reduce", worst(logits, p64.sum(1) + f64(fcr.a[1]),
                                 acc_bound(HW // 16 + 1, p64.abs().sum(1) + f64(fcr.a[1]).abs())))
    # ---- loss
    eps = n32(m["eps"])
    _bit(res, "wire_xent", "logits", xe.a[0], logits)
    _same(res, "wire_xent", "(G, bias)", tuple(xe.a[1:3]), (1, None))
    _bit(res, "wire_xent", "labels", xe.a[3], m["labels"])
    _same(res, "wire_xent", "(logits_out, dbias)", (xe.a[4], xe.a[7]), (None, None))
    _same(res, "wire_xent", "gscale = 1 / B of this batch", xe.a[8], 1.0 / B)
    _same(res, "wire_xent", "dbias scale", float(xe.a[9]), 0.0)
    _same(res, "wire_xent", "label_smoothing keyword", dict(xe.kw), {"label_smoothing": float(m["eps"])} if m["eps"] else {})
    g = n32(1.0 / B)
    lab = m["labels"]
    lg = xe.a[0]
    if eps:
        lref, dref, bl, bd = LS.bounds(lg, lab, eps, g)
    else:
        rows, p = R.xent_rows64(lg, lab)
        lref, dref = R.xent64(lg, lab, g)
        x = f64(lg)
        D = (x - x.max(1, keepdim=True).values).abs().max(1).values
        bd = g * (p * (2 * D[:, None] + 64) * U + 2 * U)
        lref, bl = lref.reshape(1), ((D + 64) * U * rows.abs().clamp(min=1.0)).mean().reshape(1)
    dl = xe.o[5]
    _upd(res, "dlogits", worst(dl, dref, bd))
    _upd(res, "loss", worst(xe.o[6].reshape(1), lref, bl))
    # ---- fc backward
    go = fcb.a[0]
    ref = f64(dl) * n32(m["scale"])
    _upd(res, "dl_scaled", worst(go, ref, U * ref.abs() + TINY))
    _bit(res, "wire_fc_bwd", "X = stored a2", fcb.a[1], a2)
    _bit(res, "wire_fc_bwd", "W = the forward's operand", fcb.a[2], fcp.a[1])
    _same(res, "wire_fc_bwd", "(scale, mask)", (float(fcb.a[5]), fcb.a[6]), (1.0, False))
    _same(res, "wire_fc_bwd", "no dbias / loss arguments", (len(fcb.a), dict(fcb.kw)), (7, {}))
    dX, dW = fcb.o[3], fcb.o[4]
    _same(res, "wire_fc_bwd", "dX dtype", None if dX is None else dX.dtype, dt)
    rdx, rdw, _ = R.fc_bwd64(go, fcb.a[1], fcb.a[2], 1.0, False)
    adx, adw, _ = R.fc_bwd64(f64(go).abs(), f64(fcb.a[1]).abs(), f64(fcb.a[2]).abs(), 1.0, False)
    _upd(res, "fc_dx", worst(dX, rdx, _out(rdx, acc_bound(NO, adx, f32b), dt)))
    _upd(res, "fc_dw", worst(dW, rdw, acc_bound(B + 2, adw, f32b)))
    hk = m["hooked"]
    _upd(res, "fc_db", worst(hk["fl.bias"], f64(go).sum(0), acc_bound(B, f64(go).abs().sum(0))))
    # ---- conv2 data gradient
    _bit(res, "wire_dgrad", "dy = stored dX", dg.a[0], dX)
    _bit(res, "wire_dgrad", "mask = stored a2", dg.a[1], a2)
    _bit(res, "wire_dgrad", "weight = [tap][ci][co] of w2.to(dtype) of the masters", dg.a[2],
         P["net.2.weight"].to(dt).view(C2, 9, C1).permute(1, 2, 0).contiguous())
    _same(res, "wire_dgrad", "(x mask, pxt)", (dg.a[3], dg.a[5]), (None, 2))
    dz1 = dg.o[4]
    if dg.a[1] is not None and tuple(dg.a[1].shape) == tuple(dg.a[0].shape) and tuple(dg.a[2].shape) == (9, C1, C2):
        gm = f64(dg.a[0]) * (f64(dg.a[1]) > 0)
        wd = f64(dg.a[2]).permute(2, 0, 1).reshape(C2, 3, 3, C1)
        ref, A = R.conv3x3_dgrad64(gm, wd), R.conv3x3_dgrad64(gm.abs(), wd.abs())
        _upd(res, "dz1", worst(dz1, ref, _out(ref, acc_bound(9 * C2, A, f32b), dt)))
    else:
        _upd(res, "dz1", (INF, ("no mask / weight of the shape",)))
    # ---- conv2 weight gradient
    Rr = wgrad_rows(H, B, dt)
    rows2 = B * -(-H // Rr)
    _bit(res, "wire_wgrad", "dy = stored dX", wg.a[0], dX)
    _bit(res, "wire_wgrad", "mask = stored a2", wg.a[1], a2)
    _bit(res, "wire_wgrad", "x = stored a1", wg.a[2], a1)
    _same(res, "wire_wgrad", "R", wg.a[4], Rr)
    slab2 = wg.o[3]
    _same(res, "wire_wgrad", "slab shape / dtype", (tuple(slab2.shape), slab2.dtype), ((rows2, ROW2), F32))
    gm = f64(wg.a[0]) * (f64(wg.a[1]) > 0) if wg.a[1] is not None else f64(wg.a[0])
    ref2, A2 = wgrad_rows_of(gm, wg.a[2], int(wg.a[4])), wgrad_rows_of(gm.abs(), f64(wg.a[2]).abs(), int(wg.a[4]))
    E2 = acc_bound(wgrad_nslot(W, int(wg.a[4])), A2, f32b)
    _upd(res, "w2slab", worst(slab2, ref2, E2))
    _seg_check(res, "wire_red2", red2, slab2, ROW2, NW2, C2, rows2)
    _reduced(res, ("gw2", "replay_w2", "gb2", "replay_b2"), red2, red2.a[0][0][0], ref2, E2, NW2)
    # ---- conv1 weight gradient
    rows1 = -(-B * HW // CHUNK)
    _bit(res, "wire_conv1w", "x = the forward's xf", c1w.a[0], xf)
    _same(res, "wire_conv1w", "index list / offsets", tuple(c1w.a[1:5]), (None, None, 0, 0))
    _bit(res, "wire_conv1w", "dy = stored dZ1", c1w.a[5], dz1)
    _bit(res, "wire_conv1w", "mask = stored a1", c1w.a[6], a1)
    _same(res, "wire_conv1w", "(B, H, W, Cout, chunk)", tuple(c1w.a[8:13]), (B, H, W, C1, CHUNK))
    slab1 = c1w.o[7]
    _same(res, "wire_conv1w", "slab shape / dtype", (tuple(slab1.shape), slab1.dtype), ((rows1, ROW1), F32))
    dz = f64(c1w.a[5]) * (f64(c1w.a[6]) > 0) if c1w.a[6] is not None else f64(c1w.a[5])
    xw = f64(c1w.a[0]).reshape(B, H, W)
    ref1, A1 = w1_rows_of(dz, xw, CHUNK), w1_rows_of(dz.abs(), xw.abs(), CHUNK)
    E1 = acc_bound(CHUNK, A1, f32b)
    _upd(res, "w1slab", worst(slab1, ref1, E1))
    _seg_check(res, "wire_red1", red1, slab1, ROW1, NW1, C1, rows1)
    _reduced(res, ("gw1", "replay_w1", "gb1", "replay_b1"), red1, red1.a[0][0][0], ref1, E1, NW1)
    # ---- what the Functions returned, where it landed
    if len(red2.o[0]) == 2 and len(red1.o[0]) == 2:
        for n, t in (("net.2.weight", red2.o[0][0][5]), ("net.2.bias", red2.o[0][1][5]), ("net.0.weight", red1.o[0][0][5]),
                     ("net.0.bias", red1.o[0][1][5]), ("fl.weight", dW)):
            _bit(res, "returned", n, hk[n].reshape(-1), t.reshape(-1))
    before, after = f64(m["grads_before"]), m["grads_after"]
    for n, (off, ne) in lay.items():
        s = before[off:off + ne] + f64(hk[n]).reshape(-1)
        _upd(res, "landing", worst(after[off:off + ne], s, U * s.abs() + TINY), n)
    gap = after[~inside_mask(lay, total)]
    _upd(res, "gaps", (0.0, ()) if not bool((gap != 0).any()) else (INF, (int(torch.nonzero(gap != 0)[0]),)))
    if m.get("gx") is not None:
        ref = R.conv3x3_dgrad64(dz, f64(P["net.0.weight"])).reshape(m["gx"].shape)
        rel = ((f64(m["gx"]) - ref).norm() / ref.norm()).item()
        _upd(res, "input_grad", (rel / 1e-5 if math.isfinite(rel) else INF, ()))


def check_step(rec):
    """{stage: (largest error / bound over every element and pass, (what, index))} of one step record."""
    res = {}
    try:
        sts, sgd = parse_trace(rec["trace"], len(rec["micro"]))
    except OrderError as e:
        return {"order": (INF, (str(e),))}
    res["order"] = (0.0, ())
    lay, total = flat_layout()
    _same(res, "layout", "layout", (dict(rec["layout"]), rec["total"]), (lay, total))
    if failing(res):
        return res
    for k, (st, m) in enumerate(zip(sts, rec["micro"])):
        check_pass(st, m, rec, res, k == 0)
    # ---- optimizer
    hp, first = rec["hp"], rec["first_step"]
    _bit(res, "wire_sgd", "parameters = the masters", sgd.a[0], to_flat(rec["params"], lay, total))
    _bit(res, "wire_sgd", "gradients = the buffer after the last backward", sgd.a[1], rec["micro"][-1]["grads_after"])
    _bit(res, "wire_sgd", "momentum buffer", sgd.a[2], torch.zeros(total) if first else rec["momentum_before"])
    _same(res, "wire_sgd", "(lr, momentum, dampening, weight decay, nesterov, maximize, first_step, update)",
          tuple(sgd.a[3:11]), (hp["lr"], hp["momentum"], 0, hp["weight_decay"], False, False, first, True))
    _same(res, "wire_sgd", "(shadows, clip, schedule)", (list(sgd.a[11]), sgd.a[12], sgd.a[13]), ([], None, None))
    a = dict(lr=n32(hp["lr"]), momentum=n32(hp["momentum"]), dampening=0.0, wd=n32(hp["weight_decay"]), nesterov=False)
    p0, g64 = f64(sgd.a[0]), f64(sgd.a[1])
    m0 = torch.zeros_like(p0) if first else f64(sgd.a[2])
    pref, bref = R.sgd64(p0, g64, m0, first_step=first, **a)
    bp, bb = K.sgd_bounds(p0, g64, m0, first_step=first, **a)
    res["param"] = worst(sgd.o[0], pref, bp)
    res["momentum"] = worst(sgd.o[2], bref, bb)
    out = ~inside_mask(lay, total)
    bad = bool((sgd.o[0][out] != 0).any()) or bool((sgd.o[2][out] != 0).any())
    res["state_gaps"] = (INF, ("a gap of the parameters / momentum is not 0",)) if bad else (0.0, ())
    return res


# ------------------------------------------------------------------------------- emulation
PLANTS = ("nominal_batch", "mask_from_a1", "wgrad_unmasked", "wt_swapped", "fc_nchw", "row_dropped", "gb2_offset",
          "landing_shifted", "biases_swapped", "accum_overwrites", "no_half_scale", "smooth_other_classes",
          "step2_momentum_init", "stale_w2")


def _nan(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype)


def _reduce32(rows32, drop_last=False):
    rows32 = rows32[:-1] if drop_last else rows32
    return torch.from_numpy(K.replay_reduce(rows32.numpy(), K.reduce_groups([rows32.shape[0]] * 2)))


def emulate_pass(P, x, u8, labels, dt, eps, scale, grads, lay, total, plant=None, stale=None, nominal=None):
    """(the 11 Calls, the pass's record) of one forward + backward in float32 / ``dt``; ``grads``
    (flat) is added onto in place.  ``stale``: the masters of the step before (plant stale_w2);
    ``nominal``: the loader's nominal batch (plant nominal_batch)."""
    T = []
    B = labels.shape[0]
    if u8 is not None:
        x = (u8.float() / 255.0).unsqueeze(1)
    xf = x.reshape(B, HW).float().contiguous()
    w1, b1, w2, b2, wfc, bfc = (P[n] for n in NAMES)
    a1 = R.conv1_relu(xf.view(B, H, W), w1, b1).to(dt)
    T.append(Call("conv1_fwd", [xf, None, None, 0, 0, w1, b1, _nan(B, H, W, C1, dtype=dt), B, H, W],
                  [xf, None, None, 0, 0, w1, b1, a1, B, H, W]))
    wb = (stale["net.2.weight"] if plant == "stale_w2" and stale is not None else w2).to(dt)
    a2 = R.conv3x3(a1.float(), wb.float(), b2, True).to(dt)
    T.append(Call("conv3x3_fwd", [a1, wb, b2, _nan(B, H, W, C2, dtype=dt), True, None, None, 0, 2],
                  [a1, wb, b2, a2, True, None, None, 0, 2]))
    fb = wfc.to(dt)
    if plant == "fc_nchw":
        fb = fb.permute(0, 2, 1).contiguous().view(NO, HW, C2)
    part = torch.einsum("bgk,ogk->bgo", a2.float().reshape(B, HW // 16, 16 * C2), fb.float().reshape(NO, HW // 16, 16 * C2))
    T.append(Call("fc_partial", [a2, fb, _nan(B, HW // 16, NO)], [a2, fb, part]))
    logits = part.sum(1) + bfc
    T.append(Call("fc_reduce", [part, bfc, _nan(B, NO), B, HW // 16, NO], [part, bfc, logits, B, HW // 16, NO]))
    gs = 1.0 / (nominal if plant == "nominal_batch" and nominal else B)
    loss, dl = LS.emulate(logits, labels, n32(eps), n32(gs), "other_classes" if plant == "smooth_other_classes" else "kernel")
    kw = {"label_smoothing": float(eps)} if eps else {}
    T.append(Call("xent", [logits, 1, None, labels, None, _nan(B, NO), _nan(1), None, gs, 0.0],
                  [logits, 1, None, labels, None, dl, loss, None, gs, 0.0], kw, kw))
    go = dl if plant == "no_half_scale" else dl * n32(scale)
    dX = (go @ fb.float().reshape(NO, -1)).view(B, H, W, C2).to(dt)
    dW = (go.t() @ a2.float().reshape(B, -1)).view(NO, HW, C2)
    T.append(Call("fc_bwd", [go, a2, fb, _nan(B, H, W, C2, dtype=dt), _nan(NO, HW, C2), 1.0, False],
                  [go, a2, fb, dX, dW, 1.0, False]))
    db = go.sum(0)
    wt = wb.view(C2, 9, C1).permute(1, 2, 0).contiguous()
    if plant == "wt_swapped":
        wt = wb.view(C2, 9, C1).permute(1, 0, 2).contiguous().view(9, C1, C2)
    mask = torch.cat([a1, a1], -1) if plant == "mask_from_a1" else a2
    dz1 = R.conv3x3_dgrad(dX.float() * (mask > 0), wt.permute(2, 0, 1).reshape(C2, 3, 3, C1).float()).to(dt)
    T.append(Call("conv3x3_dgrad", [dX, mask, wt, None, _nan(B, H, W, C1, dtype=dt), 2], [dX, mask, wt, None, dz1, 2]))
    Rr = wgrad_rows(H, B, dt)
    wmask = None if plant == "wgrad_unmasked" else a2
    gm = dX.float() * (a2 > 0) if wmask is not None else dX.float()
    slab2 = wgrad_rows_of(gm, a1, Rr, torch.float32)
    T.append(Call("conv3x3_wgrad", [dX, wmask, a1, _nan(*slab2.shape), Rr], [dX, wmask, a1, slab2, Rr]))
    off_b = NW2 - C2 if plant == "gb2_offset" else NW2
    gw2 = _reduce32(slab2[:, :NW2], plant == "row_dropped")
    gb2 = _reduce32(slab2[:, off_b:off_b + C2], plant == "row_dropped")
    rows2 = slab2.shape[0]
    seg = lambda gw, gb: [(slab2, ROW2, 0, NW2, rows2, gw, 1.0), (slab2, ROW2, off_b, C2, rows2, gb, 1.0)]  # noqa: E731
    T.append(Call("grad_reduce", [seg(_nan(NW2), _nan(C2))], [seg(gw2, gb2)]))
    slab1 = w1_rows_of(dz1.float() * (a1 > 0), xf.view(B, H, W), CHUNK, torch.float32)
    T.append(Call("conv1_wgrad", [xf, None, None, 0, 0, dz1, a1, _nan(*slab1.shape), B, H, W, C1, CHUNK],
                  [xf, None, None, 0, 0, dz1, a1, slab1, B, H, W, C1, CHUNK]))
    gw1, gb1 = _reduce32(slab1[:, :NW1]), _reduce32(slab1[:, NW1:])
    rows1 = slab1.shape[0]
    seg = lambda gw, gb: [(slab1, ROW1, 0, NW1, rows1, gw, 1.0), (slab1, ROW1, NW1, C1, rows1, gb, 1.0)]  # noqa: E731
    T.append(Call("grad_reduce", [seg(_nan(NW1), _nan(C1))], [seg(gw1, gb1)]))
    hooked = {"net.0.weight": gw1.view(SHAPES["net.0.weight"]), "net.0.bias": gb1, "net.2.weight": gw2.view(SHAPES["net.2.weight"]),
              "net.2.bias": gb2, "fl.weight": dW, "fl.bias": db}
    before = grads.clone()
    if plant == "accum_overwrites":
        grads.zero_()
    for n, (off, ne) in lay.items():
        v = hooked[n].reshape(-1)
        if plant == "landing_shifted" and n == "net.2.bias":
            off += ALIGN
        if plant == "biases_swapped" and n in ("net.0.bias", "net.2.bias"):
            other = hooked["net.2.bias" if n == "net.0.bias" else "net.0.bias"].reshape(-1)
            k = min(ne, other.numel())
            grads[off:off + k] += other[:k]
            continue
        grads[off:off + ne] += v
    rec = dict(x=x, u8=u8, labels=labels, scale=scale, eps=eps, hooked=hooked, grads_before=before, grads_after=grads.clone(),
               gx=None)
    return T, rec


def emulate_sgd(P, grads, mom, hp, first, lay, total, plant_first=False):
    p = to_flat(P, lay, total)
    m = torch.zeros(total) if mom is None else mom
    init = first or plant_first
    d = grads + p * n32(hp["weight_decay"])
    buf = d.clone() if init else m * n32(hp["momentum"]) + d
    pn = p - buf * n32(hp["lr"])
    args = [hp["lr"], hp["momentum"], 0, hp["weight_decay"], False, False, init, True, [], None, None]
    call = Call("sgd", [p, grads.clone(), m.clone()] + args, [pn, grads.clone(), buf] + args)
    newP = {n: pn[o:o + k].view(SHAPES[n]).clone() for n, (o, k) in lay.items()}
    return call, newP, buf


@functools.lru_cache(maxsize=None)
def emulate_case(case, plant=None):
    """[step record] of an emulated case.  Shared: do not write."""
    cs = CASES[case]
    lay, total = flat_layout()
    P, mom, stale, out = masters(), None, None, []
    inputs = case_inputs(case)
    if cs["loader"]:  # the loader's batches of a 17-image set in storage order: 10, then the last 7
        u8, labels = loader_dataset()
        inputs = [[(None, u8[:10], labels[:10])], [(None, u8[10:], labels[10:])]]
    for si, passes in enumerate(inputs):
        grads, T, micro = torch.zeros(total), [], []
        for x, u8b, labels in passes:
            t, m = emulate_pass(P, x, u8b, labels, cs["dtype"], cs["eps"], 1.0 / cs["accum"], grads, lay, total,
                                plant if not (plant == "accum_overwrites" and not micro) else None, stale,
                                10 if cs["loader"] else None)
            T += t
            micro.append(m)
        call, newP, buf = emulate_sgd(P, grads, mom, HP, si == 0, lay, total, plant == "step2_momentum_init")
        out.append(dict(trace=T + [call], params=P, momentum_before=mom, first_step=si == 0, dtype=cs["dtype"],
                        layout=lay, total=total, hp=HP, micro=micro))
        stale, P, mom = P, newP, buf
    return out
