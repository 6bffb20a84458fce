"""One bf16 SimpleCNN engine step, stage by stage and element by element, against float64
(tests/test_engine_step_elementwise_gpu.py runs the engine through it,
tests/test_engine_step_bounds_cpu.py shows that it admits a correct step and rejects wrong
ones).  A helper module, not a test module; it needs no GPU.

``check_step`` is teacher-forced: the float64 reference of a stage (ddp_amd/ops/reference.py) is
computed from exactly the tensors the engine stored for the stage before it - ReLU masks from
the stored bf16 a1 / a2, gradients from the stored dZ tensors - so a mask flip or an upstream
rounding never enters a later stage.  This is the method of
tests/test_simplecnn_kernels_elementwise_gpu.py applied to what engine.cpp launch_step_t wires
together: the batch it gathers, 1 / B of a ragged batch, the slab counts wgrad_rows implies,
the shadows the previous step left, loss_hist[step], the offsets of the flat gradient buffer.

Bounds (ddp_amd/ops/kernel_bounds.py; nothing is calibrated on the engine).  u = 2**-24, n =
accumulated terms, A = the operation on absolute values; fp32 outputs E = 2 n u A, bf16
outputs 2**-8 (|ref| + E) + E.  The term counts are the ones counted from the kernels in the
per-kernel suite's docstring:

  shadows     w2_bf16, w2t_bf16 ([tap][ci][co]), wfc_frag (FCFRAG order) and - on the chains that
              keep it fresh - wfc_bf16 are, bit for bit, the bf16 round-to-nearest-even of the
              masters before the step at kernel_bounds.shadow_index
  a1          conv1 of x_u8[idx] / 255 with the master w1, b1: n = 11, bf16 store
  a2          conv2 of the stored a1 with bf16(w2), b2: n = 9 * 32 + 1, bf16 store
  fc_part     (levels 0, 1) per block of CH = 64 pxt pixels from the stored a2: n = 64 CH + CH / 4
  dlogits,    kernel_bounds.xent_rows_bounds with gscale = fl32(1 / B).  End to end: logits =
  loss_rows   fc64(stored a2, bf16(wfc), bfc) with e_l = 2 n u A, n = HW C + HW / 16 + 1 (a block
              partial's 64 CH + CH / 4 terms and the fold's HW / CH + 2 adds lie inside it).
              Where fc_part is stored also the tighter form: logits = the fold of the STORED
              partials + bias, e_l = 2 G u (sum |part| + |bias|), G = partials per logit + 1
  loss_hist   slot k = the mean of the stored loss_rows: n = B + 1; every other slot keeps its bits
  dz2         fc_bwd dX from the stored dlogits, bf16(wfc), mask a2 > 0: n = 10, bf16 store;
              masked elements are exactly 0
  dz1         (level 0) dgrad of the stored dz2 with bf16(w2), mask a1 > 0: n = 9 * 64, bf16 store;
              masked elements exactly 0
  grad wfc,   scale * dlogits^T a2 and scale * sum_b dlogits from the stored tensors, scale =
  grad bfc    1 / world: n = B + 2
  w2slab      row (image, chunk of R output rows) from the stored dz2, a1: n = nslot =
              roundup32(R roundup8(W)); the rows are those conv3x3_wgrad_blocks(B, 28, R) counts
  grad w2,b2  the sum of the float64 rows: the row bounds summed + the reducer's
              2 (rows + 2) u sum |stored row|
  w1slab      row = block of CH1 = 64 pxt_dgrad pixels of the stored dz1 against x: n = CH1 + 9
  grad w1,b1  the row bounds summed + the reducer term, as conv2's
  params,     R.sgd64 of the masters (and momentum) before with the STORED gradient where the
  momentum    chain stores it: kernel_bounds.sgd_bounds; where it does not (the fused optimizer
              consumes the fc weight gradient in registers) with the float64 gradient: sgd_bounds
              + lr * (the gradient's bound) for the parameter, + |1 - dampening| * (the
              gradient's bound) for the momentum buffer (the whole bound on its first step)

Stages a chain does not materialise are replaced by their float64 value and its bound is
carried into the stages that read it (first order in the carried error, exact in the rest):

  no dz1 (level >= 1: the dgrad role keeps the bf16-rounded dZ1 in registers): d = the float64
     dgrad of the stored dz2, e1 = its bf16-store bound; a slab row from the rounded values is
     within 2 (CH1 + 9) u sum (|d| + e1) x of their exact sum, which is within sum e1 x of the row
     of d: row bound = 2 (CH1 + 9) u sum (|d| + e1) x + sum e1 x.
  no dlogits / loss_rows (level 1: fc_bwd's prologue keeps them in LDS): dL = the float64
     cross-entropy of the stored partials, e_d its xent_rows bound; dz2's accumulation bound
     grows by sum_o e_d |wfc|, the fc gradients' by scale * sum_b e_d |a2| and scale * sum_b e_d,
     and loss_hist's reference is the mean of the float64 row losses with the mean of their
     bounds added.

``emulate_step`` is an fp32 / bf16 model of the same stages (torch's float32 operators, bf16
roundings at the engine's store points, as R.simple_cnn_step_bf16, whose results it must keep
reproducing) that also returns the intermediates; its keyword arguments plant the wiring
errors the CPU test wants rejected.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from ddp_amd.ops import kernel_bounds as K
from ddp_amd.ops import reference as R
from ddp_amd.ops.kernel_bounds import U, acc_bound, bf16_store_bound

BF = torch.bfloat16
H = W = 28
HW, C1, C2, NO = H * W, 32, 64, 10
N_W2, N_FC = C2 * 9 * C1, NO * HW * C2
PARAMS = ("w1", "b1", "w2", "b2", "wfc", "bfc")
SHAPES = {"w1": (C1, 3, 3, 1), "b1": (C1,), "w2": (C2, 3, 3, C1), "b2": (C2,), "wfc": (NO, HW, C2), "bfc": (NO,)}
# the order the stages depend on each other in: a planted error is "caught at its stage" when
# that stage is the first of these that fails
STAGES = ("shadows", "a1", "a2", "fc_part", "dlogits", "loss_rows", "dlogits_part", "loss_rows_part", "loss_hist",
          "dz2", "dz1", "grad_wfc", "grad_bfc", "w2slab", "grad_w2", "grad_b2", "w1slab", "grad_w1", "grad_b1") + \
    tuple(f"param_{k}" for k in PARAMS) + tuple(f"momentum_{k}" for k in PARAMS)


def n32(v):
    return float(np.float32(v))


def make_plan(B, level=0, pxt_fwd=1, pxt_dgrad=2, wgrad_rows=None, max_batch=None, k=0, lr=0.01, momentum=0.0,
              dampening=0.0, weight_decay=0.0, nesterov=False, first_step=True, world=1, plain_fc_fresh=None):
    """What check_step needs to know about the chain that ran.  ``k``: the step's index in its
    epoch (its loss_hist slot); ``wgrad_rows``: the engine's R, chosen for ``max_batch``
    (functional.wgrad_rows when None); ``first_step``: the momentum buffer's initialising step;
    ``plain_fc_fresh``: whether wfc_bf16 is kept current (not on the level-3 chain)."""
    mb = max_batch or B
    if wgrad_rows is None:
        wgrad_rows = next((r for r in (7, 4, 2, 1) if mb * -(-H // r) >= 128), 1)
    return dict(B=B, level=level, CH=64 * pxt_fwd, CH1=64 * pxt_dgrad, R=wgrad_rows, max_batch=mb, k=k, lr=n32(lr),
                momentum=n32(momentum), dampening=n32(dampening), wd=n32(weight_decay), nesterov=bool(nesterov),
                first_step=bool(first_step), world=world,
                plain_fc_fresh=(level < 3) if plain_fc_fresh is None else plain_fc_fresh)


def f64(t):
    return t.detach().cpu().double()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def bf(t):
    return t.detach().cpu().float().to(BF)


def shadow_of(master, kind, a=0, b=0, c=0):
    """The bf16 shadow of a flat fp32 master in layout ``kind`` (kernel_bounds.shadow_index)."""
    flat = master.detach().cpu().float().reshape(-1)
    out = torch.zeros(K.shadow_dst_numel(kind, flat.numel()), dtype=BF)
    out[torch.from_numpy(K.shadow_index(kind, flat.numel(), a, b, c))] = flat.to(BF)
    return out


def entry_shadows(before):
    return {"w2_bf16": shadow_of(before["w2"], K.SHADOW_BF16),
            "w2t_bf16": shadow_of(before["w2"], K.SHADOW_BF16_TAPT, C2, 9, C1),
            "wfc_frag": shadow_of(before["wfc"], K.SHADOW_BF16_FCFRAG, HW, C2),
            "wfc_bf16": shadow_of(before["wfc"], K.SHADOW_BF16)}


def nslot(R_):
    return (R_ * ((W + 7) & ~7) + 31) // 32 * 32


def wgrad_rows_of(dy, x, R_, dtype=torch.float64):
    """conv3x3_wgrad's slab rows [B * ceil(H / R)][Co * 9 * Ci + Co] in ``dtype``: row = image n,
    chunk c of R output rows - (dW OHWI, db) of those rows alone."""
    dy, x = dy.detach().cpu().to(dtype), x.detach().cpu().to(dtype)
    B = dy.shape[0]
    nRC = -(-H // R_)
    sh = [R._shift(x, kh - 1, kw - 1) for kh in range(3) for kw in range(3)]
    rows = torch.zeros(B, nRC, N_W2 + C2, dtype=dtype)
    for c in range(nRC):
        r0, r1 = c * R_, min(H, (c + 1) * R_)
        d = dy[:, r0:r1]
        dw = torch.stack([torch.einsum("nhwo,nhwi->noi", d, s[:, r0:r1]) for s in sh], 2)  # [B,Co,9,Ci]
        rows[:, c, :N_W2] = dw.reshape(B, -1)
        rows[:, c, N_W2:] = d.sum(dim=(1, 2))
    return rows.reshape(B * nRC, -1)


def w1_rows_of(dz, x01, CH1, dtype=torch.float64):
    """The fused conv1 weight gradient's slab rows [blocks][32 * 9 + 32] in ``dtype``: block k =
    the flattened pixels [k CH1, (k + 1) CH1) of dZ1 [B,H,W,32] against the image taps x01
    [B,H,W] (already / 255) - (dW [co][tap], db)."""
    dz, x01 = dz.detach().cpu().to(dtype), x01.detach().cpu().to(dtype)
    B = dz.shape[0]
    taps = torch.stack([R._shift(x01.unsqueeze(-1), kh - 1, kw - 1)[..., 0] for kh in range(3) for kw in range(3)], -1)
    nblk = -(-B * HW // CH1)
    pad = nblk * CH1 - B * HW
    d = F.pad(dz.reshape(B * HW, C1), (0, 0, 0, pad)).view(nblk, CH1, C1)
    t = F.pad(taps.reshape(B * HW, 9), (0, 0, 0, pad)).view(nblk, CH1, 9)
    dw = torch.einsum("kpc,kpt->kct", d, t).reshape(nblk, C1 * 9)
    return torch.cat([dw, d.sum(1)], 1)


def fold_terms(b, CH):
    """(block, slot) of every partial summed into image b's logits (common.h xent_logit_idx)."""
    p0 = b * HW
    kb0, kb1 = p0 // CH, (p0 + HW - 1) // CH
    return [(kb0 + j, (0 if kb0 * CH == p0 else 1) if j == 0 else 0) for j in range(kb1 - kb0 + 1)]


def worst(out, ref, bound, exact_zero=None):
    """(max |out - ref| / bound, index of the worst element); a non-finite output or a non-zero
    element under ``exact_zero`` counts as infinitely far out."""
    o = f64(out)
    assert o.shape == ref.shape, (o.shape, ref.shape)
    rr = (o - ref).abs() / (bound + 1e-300)
    rr = torch.where(torch.isfinite(o), rr, torch.full_like(rr, float("inf")))
    if exact_zero is not None:
        rr = torch.where(exact_zero & (o != 0), torch.full_like(rr, float("inf")), rr)
    if rr.numel() == 0:
        return 0.0, ()
    i = int(rr.reshape(-1).argmax())
    return rr.reshape(-1)[i].item(), tuple(int(v) for v in np.unravel_index(i, tuple(rr.shape)))


def bitwise(out, want):
    """(0 or inf, first differing index): a stage that must match bit for bit."""
    a, b = bits(out).reshape(-1), bits(want).reshape(-1)
    if a.shape != b.shape:
        return float("inf"), ()
    d = torch.nonzero(a != b)
    return (0.0, ()) if d.numel() == 0 else (float("inf"), (int(d[0]),))


def _xent(x, absum, G, labels, gscale):
    rl, p = R.xent_rows64(x, labels)
    _, dref = R.xent64(x, labels, gscale)
    bd, bl = K.xent_rows_bounds(x, absum, G, labels, gscale, p, rl)
    return dref, rl, bd, bl


def check_step(obs, before, x_u8, labels, B, plan):
    """{stage: (largest error / bound, index of the worst element)} for the stages present in
    ``obs`` (see the module docstring).  ``obs``: CPU tensors by name - the entry shadows, a1, a2,
    fc_part, dlogits, loss_rows, loss_hist (+ loss_hist_before), dz2, dz1, w2slab, w1slab, grads
    {name: tensor}, params_after {name: tensor}, momentum_before / momentum_after {name: tensor}.
    ``before``: the fp32 masters before the step; ``x_u8`` [B,28,28] uint8 and ``labels`` [B]: the
    step's batch, gathered by the caller from the sampler's index list."""
    res = {}
    x_u8, labels = x_u8.detach().cpu(), labels.detach().cpu().long()
    assert x_u8.shape == (B, H, W) and labels.shape == (B,)
    P = {k: before[k].detach().cpu().float().reshape(SHAPES[k]) for k in PARAMS}
    w2b, wfcb = bf(P["w2"]), bf(P["wfc"])
    scale = n32(1.0 / plan["world"])
    gscale = n32(np.float32(1.0) / np.float32(B))

    # ---- shadows at step entry
    want = entry_shadows(P)
    sh = [bitwise(obs[k], want[k]) for k in ("w2_bf16", "w2t_bf16", "wfc_frag") if k in obs]
    if plan["plain_fc_fresh"] and "wfc_bf16" in obs:
        sh.append(bitwise(obs["wfc_bf16"], want["wfc_bf16"]))
    if sh:
        res["shadows"] = max(sh, key=lambda t: t[0])

    # ---- forward
    a1 = obs["a1"].reshape(-1)[:B * HW * C1].view(B, H, W, C1) if "a1" in obs else None
    a2 = obs["a2"].reshape(-1)[:B * HW * C2].view(B, H, W, C2)
    if a1 is not None:
        ref = R.conv1_64(x_u8, P["w1"].reshape(C1, 9), P["b1"])
        A = R.conv3x3_64((f64(x_u8) / 255.0).unsqueeze(-1), f64(P["w1"]).abs(), f64(P["b1"]).abs())
        res["a1"] = worst(a1, ref, bf16_store_bound(ref, acc_bound(11, A)))
    else:  # (a chain that never stores a1: the float64 conv1, rounded as the kernel stores it)
        a1 = bf(R.conv1_64(x_u8, P["w1"].reshape(C1, 9), P["b1"]))
    ref = R.conv3x3_64(a1, w2b, P["b2"], True)
    A = R.conv3x3_64(a1.abs(), w2b.abs(), P["b2"].abs())
    res["a2"] = worst(a2, ref, bf16_store_bound(ref, acc_bound(9 * C1 + 1, A)))

    # ---- logits, cross-entropy
    xe = R.fc64(a2, wfcb, P["bfc"])
    Ae = R.fc64(a2.abs(), wfcb.abs(), P["bfc"].abs())
    dl_ref, rl_ref, bd, bl = _xent(xe, Ae, HW * C2 + HW // 16 + 1, labels, gscale)
    if "fc_part" in obs:
        CH = plan["CH"]
        nblk = -(-B * HW // CH)
        part = obs["fc_part"].reshape(-1)[:nblk * 2 * NO].view(nblk, 2, NO)
        pref = R.fc_block_partials64(a2, wfcb, CH)
        pA = R.fc_block_partials64(a2.abs(), wfcb.abs(), CH)
        res["fc_part"] = worst(part, pref, acc_bound(64 * CH + CH // 4, pA))
        terms = [fold_terms(b, CH) for b in range(B)]
        p64, b64 = f64(part), f64(P["bfc"])
        xp = torch.stack([sum(p64[k, s] for k, s in terms[b]) + b64 for b in range(B)])
        ap = torch.stack([sum(p64[k, s].abs() for k, s in terms[b]) + b64.abs() for b in range(B)])
        dl_p, rl_p, bd_p, bl_p = _xent(xp, ap, max(len(t) for t in terms) + 1, labels, gscale)
    if "dlogits" in obs:
        dl = obs["dlogits"].reshape(-1)[:B * NO].view(B, NO)
        res["dlogits"] = worst(dl, dl_ref, bd)
        if "fc_part" in obs:
            res["dlogits_part"] = worst(dl, dl_p, bd_p)
        dl64, e_d = f64(dl), None
    else:  # carried: the float64 dL of the stored partials (of the stored a2 without them)
        dl64, e_d = (dl_p, bd_p) if "fc_part" in obs else (dl_ref, bd)
    if "loss_rows" in obs:
        lrows = obs["loss_rows"].reshape(-1)[:B]
        res["loss_rows"] = worst(lrows, rl_ref, bl)
        if "fc_part" in obs:
            res["loss_rows_part"] = worst(lrows, rl_p, bl_p)
        l64, e_l = f64(lrows), 0.0
    else:
        l64, e_l = (rl_p, bl_p.mean()) if "fc_part" in obs else (rl_ref, bl.mean())
    if "loss_hist" in obs:
        k, hist = plan["k"], obs["loss_hist"].reshape(-1)
        ref = l64.mean().reshape(1)
        bound = acc_bound(B + 1, l64.abs().mean().reshape(1) + e_l) + e_l
        r = worst(hist[k:k + 1], ref, bound)
        if "loss_hist_before" in obs:  # every other slot keeps its bits
            keep = torch.ones(hist.numel(), dtype=torch.bool)
            keep[k] = False
            rb = bitwise(hist[keep], obs["loss_hist_before"].reshape(-1)[keep])
            r = max(r, rb, key=lambda t: t[0])
        res["loss_hist"] = r

    # ---- fc backward
    dz2 = obs["dz2"].reshape(-1)[:B * HW * C2].view(B, H, W, C2)
    keep2 = f64(a2) > 0
    ref, _, _ = R.fc_bwd64(dl64, a2, wfcb, 1.0, True)
    A, _, _ = R.fc_bwd64(dl64.abs(), a2, wfcb.abs(), 1.0, True)
    E = acc_bound(NO, A)
    if e_d is not None:
        E = E + R.fc_bwd64(e_d, a2, wfcb.abs(), 1.0, True)[0]
    res["dz2"] = worst(dz2, ref, bf16_store_bound(ref, E), exact_zero=~keep2)
    _, gw, gb = R.fc_bwd64(dl64, a2, wfcb, scale, False)
    _, Aw, Ab = R.fc_bwd64(dl64.abs(), a2.abs(), wfcb, scale, False)
    Ew, Eb = acc_bound(B + 2, Aw), acc_bound(B + 2, Ab)
    if e_d is not None:
        _, cw, cb = R.fc_bwd64(e_d, a2.abs(), wfcb, scale, False)
        Ew, Eb = Ew + cw, Eb + cb
    gref = {"wfc": (gw, Ew), "bfc": (gb, Eb)}

    # ---- conv backward
    keep1 = f64(a1) > 0
    d1 = R.conv3x3_dgrad64(dz2, w2b) * keep1
    E1 = bf16_store_bound(d1, acc_bound(9 * C2, R.conv3x3_dgrad64(dz2.abs(), w2b.abs()) * keep1))
    x01 = f64(x_u8) / 255.0
    CH1 = plan["CH1"]
    if "dz1" in obs:
        dz1 = obs["dz1"].reshape(-1)[:B * HW * C1].view(B, H, W, C1)
        res["dz1"] = worst(dz1, d1, E1, exact_zero=~keep1)
        r1 = w1_rows_of(dz1, x01, CH1)
        E1r = acc_bound(CH1 + 9, w1_rows_of(dz1.abs(), x01, CH1))
    else:
        r1 = w1_rows_of(d1, x01, CH1)
        E1r = acc_bound(CH1 + 9, w1_rows_of(d1.abs() + E1, x01, CH1)) + w1_rows_of(E1, x01, CH1)
    r2 = wgrad_rows_of(dz2, a1, plan["R"])
    E2r = acc_bound(nslot(plan["R"]), wgrad_rows_of(dz2.abs(), a1.abs(), plan["R"]))
    for name, rows, Er, nw, gw_, gb_ in (("w2slab", r2, E2r, N_W2, "w2", "b2"), ("w1slab", r1, E1r, C1 * 9, "w1", "b1")):
        tot = Er.sum(0)
        if name in obs:
            slab = obs[name].reshape(-1)[:rows.numel()].view(rows.shape)
            res[name] = worst(slab, rows, Er)
            tot = tot + K.reduce_bound(f64(slab), scale)
        else:
            tot = tot + K.reduce_bound(rows.abs() + Er, scale)
        g = scale * rows.sum(0)
        gref[gw_] = (g[:nw].reshape(SHAPES[gw_]), scale * tot[:nw].reshape(SHAPES[gw_]))
        gref[gb_] = (g[nw:], scale * tot[nw:])

    # ---- the gradients in the flat buffer, the optimizer
    grads = obs.get("grads", {})
    for k in PARAMS:
        if k in grads:
            res[f"grad_{k}"] = worst(grads[k].reshape(SHAPES[k]), gref[k][0].reshape(SHAPES[k]), gref[k][1].reshape(SHAPES[k]))
    after, m_before, m_after = obs.get("params_after", {}), obs.get("momentum_before", {}), obs.get("momentum_after", {})
    a = dict(lr=plan["lr"], momentum=plan["momentum"], dampening=plan["dampening"], wd=plan["wd"], nesterov=plan["nesterov"])
    for k in PARAMS:
        if k not in after:
            continue
        first = plan["first_step"]
        p0 = f64(P[k])
        if k in grads:  # what sgd_one consumed is what the chain stored
            g, eg = f64(grads[k]).reshape(SHAPES[k]), 0.0
        else:
            g, eg = gref[k][0].reshape(SHAPES[k]), gref[k][1].reshape(SHAPES[k])
        mom = plan["momentum"] != 0.0
        m0 = f64(m_before[k]).reshape(SHAPES[k]) if (mom and not first) else torch.zeros_like(p0)
        pref, bref = R.sgd64(p0, g, m0, first_step=first, **a)
        bp, bb = K.sgd_bounds(p0, g.abs() + eg, m0, first_step=first, **a)
        # the gradient's error reaches the buffer through (1 - dampening) (whole on its first
        # step) and the parameter through lr times that (nesterov: once more through momentum)
        cb = eg if (first or not mom) else abs(1.0 - a["dampening"]) * eg
        cd = eg + abs(a["momentum"]) * cb if (mom and a["nesterov"]) else cb
        res[f"param_{k}"] = worst(after[k].reshape(SHAPES[k]), pref, bp + a["lr"] * cd)
        if mom and k in m_after:
            res[f"momentum_{k}"] = worst(m_after[k].reshape(SHAPES[k]), bref, bb + cb)
    return res


def failing(res):
    """The stages out of bound, in dependency order."""
    return [s for s in STAGES if s in res and not res[s][0] <= 1.0]


def report(res, chain, B, tag="STEP_RATIO"):
    for s in STAGES:
        if s in res:
            print(f"{tag} {chain} {B} {s} {res[s][0]:.3e}")


# ------------------------------------------------------------------------------- emulation
def _sgd32(p, g, m, a, first):
    """torch.optim.SGD's sequence of operations in float32 (another order of roundings than
    sgd_one's fma chain)."""
    f = np.float32
    d = g + f(a["wd"]) * p if a["wd"] else g.clone()
    buf = None
    if a["momentum"]:
        buf = d.clone() if first else m * f(a["momentum"]) + d * f(1.0 - a["dampening"])
        d = d + buf * f(a["momentum"]) if a["nesterov"] else buf
    return p - d * f(a["lr"]), buf


def emulate_step(before, x_u8, labels, B, plan=None, momentum_before=None, loss_hist_before=None,
                 drop_image=None, gscale=None, drop_w2_row=None, hist_slot=None):
    """An fp32 / bf16 model of the engine's stage outputs for the batch (x_u8 [B,28,28], labels
    [B]) from the masters ``before``: the ``obs`` of :func:`check_step`, every stage present
    (level 0 with the gradients stored and the optimizer applied).

    Planted wiring errors (tests/test_engine_step_bounds_cpu.py): ``drop_image`` - an image left
    out of every gradient sum; ``gscale`` - another cross-entropy scale than 1 / B;
    ``drop_w2_row`` - a conv2 slab row the reduction skips; ``hist_slot`` - the loss written to
    another slot than plan["k"]."""
    plan = plan or make_plan(B)
    P = {k: before[k].detach().cpu().float().reshape(SHAPES[k]) for k in PARAMS}
    x_u8, labels = x_u8.detach().cpu(), labels.detach().cpu().long()
    x = x_u8.float() / 255.0
    obs = dict(entry_shadows(P))
    w2b, wfcb = R.bf16r(P["w2"]), R.bf16r(P["wfc"])
    a1 = R.bf16r(R.conv1_relu(x, P["w1"], P["b1"]))
    a2 = R.bf16r(R.conv3x3(a1, w2b, P["b2"], relu=True))
    obs["a1"], obs["a2"] = a1.to(BF), a2.to(BF)
    # the fused fc epilogue's per-block partial logits, then their fold
    CH = plan["CH"]
    nblk = -(-B * HW // CH)
    per_px = torch.einsum("bpc,opc->bpo", a2.reshape(B, HW, C2), wfcb)  # [B,HW,NO] float32
    part = torch.zeros(nblk, 2, NO)
    for k in range(nblk):
        p0, p1 = k * CH, min((k + 1) * CH, B * HW)
        n0 = p0 // HW
        for slot in (0, 1):
            lo, hi = max(p0, (n0 + slot) * HW), min(p1, (n0 + slot + 1) * HW)
            if lo < hi:
                part[k, slot] = per_px[n0 + slot, lo - (n0 + slot) * HW:hi - (n0 + slot) * HW].sum(0)
    obs["fc_part"] = part
    logits = torch.stack([sum((part[k, s] for k, s in fold_terms(b, CH)), torch.zeros(NO)) + P["bfc"] for b in range(B)])
    lp = torch.log_softmax(logits, 1)
    rows = -lp[torch.arange(B), labels]
    d = lp.exp()
    d[torch.arange(B), labels] -= 1.0
    dl = d * np.float32(np.float32(1.0) / np.float32(B) if gscale is None else gscale)
    obs["dlogits"], obs["loss_rows"] = dl, rows
    hist = torch.zeros(plan["k"] + 3) if loss_hist_before is None else loss_hist_before.clone().float()
    obs["loss_hist_before"] = hist.clone()
    hist[plan["k"] if hist_slot is None else hist_slot] = rows.sum() / np.float32(B)
    obs["loss_hist"] = hist
    dz2 = R.bf16r((dl @ wfcb.reshape(NO, -1)).view_as(a2) * (a2 > 0))
    dz1 = R.bf16r(R.conv3x3_dgrad(dz2, w2b)) * (a1 > 0)
    obs["dz2"], obs["dz1"] = dz2.to(BF), dz1.to(BF)
    live = torch.ones(B, dtype=torch.bool)
    if drop_image is not None:
        live[drop_image] = False
    s = np.float32(1.0 / plan["world"])
    g = {"wfc": ((dl[live].t() @ a2.reshape(B, -1)[live]) * s).view(SHAPES["wfc"]), "bfc": dl[live].sum(0) * s}
    nRC = -(-H // plan["R"])
    w2slab = wgrad_rows_of(dz2, a1, plan["R"], torch.float32)
    w1slab = w1_rows_of(dz1, x, plan["CH1"], torch.float32)
    obs["w2slab"], obs["w1slab"] = w2slab, w1slab
    use2 = live.repeat_interleave(nRC)
    if drop_w2_row is not None:
        use2[drop_w2_row] = False
    r1 = w1slab if drop_image is None else w1_rows_of(dz1 * live.view(B, 1, 1, 1), x, plan["CH1"], torch.float32)
    GR = K.reduce_groups([w2slab.shape[0], w1slab.shape[0]])
    red2 = torch.from_numpy(K.replay_finish(K.replay_reduce(w2slab[use2].numpy(), GR), s))
    red1 = torch.from_numpy(K.replay_finish(K.replay_reduce(r1.numpy(), GR), s))
    g.update(w2=red2[:N_W2].view(SHAPES["w2"]), b2=red2[N_W2:], w1=red1[:C1 * 9].view(SHAPES["w1"]), b1=red1[C1 * 9:])
    obs["grads"] = g
    a = dict(lr=plan["lr"], momentum=plan["momentum"], dampening=plan["dampening"], wd=plan["wd"], nesterov=plan["nesterov"])
    obs["params_after"], obs["momentum_after"] = {}, {}
    if momentum_before is not None:
        obs["momentum_before"] = {k: momentum_before[k].detach().cpu().float().reshape(SHAPES[k]) for k in PARAMS}
    for k in PARAMS:
        m0 = obs["momentum_before"][k] if (plan["momentum"] and not plan["first_step"]) else None
        pn, buf = _sgd32(P[k], g[k].reshape(SHAPES[k]), m0, a, plan["first_step"])
        obs["params_after"][k] = pn
        if buf is not None:
            obs["momentum_after"][k] = buf
    return obs


# -------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def masters(seed=0):
    """SimpleCNN-like masters in the engine's native layouts (torch's default initialisation
    scales).  Shared: do not write what this returns."""
    g = torch.Generator().manual_seed(1000 + seed)

    def uni(shape, fan_in):
        return (torch.rand(*shape, generator=g) * 2 - 1) / fan_in ** 0.5

    return {"w1": uni(SHAPES["w1"], 9), "b1": uni(SHAPES["b1"], 9), "w2": uni(SHAPES["w2"], 9 * C1),
            "b2": uni(SHAPES["b2"], 9 * C1), "wfc": uni(SHAPES["wfc"], HW * C2), "bfc": uni(SHAPES["bfc"], HW * C2)}


@functools.lru_cache(maxsize=None)
def dataset(n=96, seed=0):
    """(images uint8 [n,28,28], labels int64 [n], an index permutation): blobs on a dark
    background, so conv1's ReLU masks are mixed."""
    g = torch.Generator().manual_seed(2000 + seed)
    img = torch.rand(n, H, W, generator=g) * (torch.rand(n, H, W, generator=g) > 0.6)
    return (img * 255).to(torch.uint8), torch.randint(0, NO, (n,), generator=g), torch.randperm(n, generator=g)
