"""One SimpleCNN engine step - bf16, or exact fp32 (the second table below) - stage by stage and
element by element, against float64 (tests/test_engine_step_elementwise_gpu.py and
tests/test_engine_step_fp32_elementwise_gpu.py run the engine through it,
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

The exact-fp32 step (``prec="fp32"``: engine.cpp launch_step_t<float>;
tests/test_engine_step_fp32_elementwise_gpu.py).  The operands are the fp32 masters themselves
(no bf() of w2 / wfc), every store is fp32 (no 2**-8 term), the products round too: every bound
is acc_bound(n, A, f32_operands=True) = 3 n u A.  The counts, and where they were counted:

  shadows     w2t_f32 ([tap][ci][co], SHADOW_F32_TAPT) and wfc_frag32 (SHADOW_F32_FCFRAG) are, bit
              for bit, the masters before the step at kernel_bounds.shadow_index
  a1          never stored (store_a1 = 0: conv1_recompute_tile in the forward's and the wgrad
              role's staging pass, conv1_eval_g in the dgrad role's mask).  Reference: the float64
              conv1, e_a1 = 3 * 11 u A (9 fma, the bias, u8 / 255: the per-kernel suite's conv1_fwd row)
  a2          conv2 of a1 with the master w2, b2: n = 9 * 32 + 1 (conv3x3_fwd_body.inc.h: the
              16x16x4 MFMA chain tap-major over the 32 channels, the bias add) on |a1| + e_a1, plus
              the float64 conv of e_a1 with |w2| (first order in the carried error)
  fc_part     (level 1) per block of CH = 64 pxt_fwd pixels (the fp32 engine resolves pxt_fwd = 2:
              CH = 128) of the stored a2 against wfc in the wfc_frag32 fragment order (fma chains of
              4 channels x 4 groups per pixel, sum16 over a tile's pixels, the fixed-order sum of CH /
              16 tiles x 4 groups): n = 16 + 4 + CH / 4 = 52, the longest chain of roundings between
              a term and the partial (a lane's 16 fma from 0, sum16's 4 levels, CH / 4 adds) - counted
              anew from conv3x3_fwd_body.inc.h: the per-kernel suite's 64 CH + CH / 4 counts every term
              of the block as if summed in one chain, 158 times this bound, and would let a
              bf16-rounded wfc through
  dlogits,    as above; stored by the level-3 forward (FwdDz dl_out / loss_rows), carried on
  loss_rows   level 1.  The end-to-end logit error is 3 n u A, n = HW C + HW / 16 + 1; the fold of
              stored partials has no products and keeps 2 G u (sum |part| + |bias|)
  loss_hist   as above
  dz2         n = 10 (level 3: the forward's fma chain o = 0..9 from 0 over the wfc_frag32 quads it
              holds; level 1: fc_bwd's dX over the plain master); masked elements (stored a2 <= 0)
              are exactly 0
  dz1         never stored: d = the float64 dgrad of the stored dz2 with the master w2 under the
              float64 conv1 mask, e1 = 3 * 9 * 64 u A where the mask keeps the element, 0 where it
              drops it (conv3x3_body.h dgrad_body: 9 taps x two 32-wide K steps of 16x16x4 MFMAs; WGS
              = 1 reads the A fragments from w2t_f32 in global memory, the chain is the same)
  grad wfc,   n = B + 2 (fc_bwd_body.h fc_dw_wave_chunk / fc_bwd_bias_loss: a fma per image, the
  grad bfc    scale), as the bf16 table
  w2slab      row (image, chunk of R rows), R = functional.wgrad_rows(28, max_batch, float32) (4, 2
              or 1), the rows conv3x3_wgrad_blocks(B, 28, R) counts: n = nslot = roundup32(R
              roundup8(W)) (wgrad_body F32: every (co, tap, ci) runs one 16x16x4 MFMA chain over
              the nslot pixel slots) on |dz2| (|a1| + e_a1), plus sum |dz2| e_a1.  wgrad_split = 2
              puts two blocks on a row, the chain unchanged: half 0 (ciT = 0) writes columns ci <
              16 of every (co, tap) and the 64 bias columns, half 1 (ciT = 16) the columns ci >= 16
  w1slab      row = block of CH1 = 64 pxt_dgrad pixels, conv3x3_dgrad_blocks(B, 28, 28, pxt_dgrad)
              rows: n = CH1 + 9 and the dz1 carry of the bf16 table without its store term.  The
              dgrad channel split (dgrad_body HALF) puts two blocks on a row: half `by` writes conv1
              channels [16 by, 16 by + 16) - columns [144 by, 144 by + 144) and bias columns 288 +
              [16 by, 16 by + 16)
  grad w1,b1, the float64 row sums under the row bounds summed + reduce_bound; and bit for bit the
  grad w2,b2  float32 replay_reduce / replay_finish of the STORED rows (stages replay_*), with
              reduce_groups of the two row counts - slab_reduce.h's order, which grad_reduce and the
              conv backward's fused reducers share
  params,     as the bf16 table
  momentum

The conv1 ReLU mask is recomputed, so it may differ from float64 where the float64
pre-activation lies inside e_a1 (the ambiguous set): there the carried dz1 bound is the unmasked
|dgrad| + its accumulation bound, whatever the float64 mask says.  check_step asserts that the
set holds at most AMBIG_CAP = 1e-4 of a1's elements.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import elementwise as EW
from ddp_amd.ops import kernel_bounds as K
from ddp_amd.ops import reference as R
from ddp_amd.ops.kernel_bounds import acc_bound, bf16_store_bound
from elementwise import BF, bf, bits, bitwise, f64, n32, worst  # noqa: F401  (reachable as E.worst, E.bits ...)

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
# the same order with the fp32 table's bitwise replay of the four reduced gradients in it
ORDER = tuple(t for s in STAGES for t in ((s, "replay_" + s[5:]) if s in ("grad_w2", "grad_b2", "grad_w1", "grad_b1") else (s,)))
AMBIG_CAP = 1e-4  # the largest share of a1 whose recomputed ReLU mask may differ from float64's
failing = functools.partial(EW.failing, order=ORDER)                  # failing(res)
report = functools.partial(EW.report, order=ORDER, tag="STEP_RATIO")  # report(res, chain, B)


def fp32_stages(level, momentum):
    """The stages of the fp32 table a step of chain ``level`` (1 or 3) with every gradient stored
    reports: fc_part where the forward stores it (level 1), dlogits and loss_rows where it
    stores them (level 3); no a1, no dz1."""
    s = {"shadows", "a2", "loss_hist", "dz2", "w2slab", "w1slab"} | {f"param_{k}" for k in PARAMS}
    s |= {"fc_part"} if level < 3 else {"dlogits", "loss_rows"}
    s |= {f"grad_{k}" for k in PARAMS} | {f"replay_{k}" for k in ("w1", "b1", "w2", "b2")}
    return s | ({f"momentum_{k}" for k in PARAMS} if momentum else set())


def make_plan(B, level=0, pxt_fwd=None, pxt_dgrad=2, wgrad_rows=None, max_batch=None, k=0, lr=0.01, momentum=0.0,
              dampening=0.0, weight_decay=0.0, nesterov=False, first_step=True, world=1, plain_fc_fresh=None,
              prec="bf16"):
    """What check_step needs to know about the chain that ran.  ``k``: the step's index in its
    epoch (its loss_hist slot); ``wgrad_rows``: the engine's R, chosen for ``max_batch``
    (functional.wgrad_rows when None); ``first_step``: the momentum buffer's initialising step;
    ``plain_fc_fresh``: whether wfc_bf16 is kept current (not on the level-3 chain); ``prec``:
    "bf16" or "fp32", the table of the module docstring the step is held to; ``pxt_fwd`` None: 1,
    for fp32 the 2 its engine resolves."""
    assert prec in ("bf16", "fp32"), prec
    mb = max_batch or B
    if pxt_fwd is None:
        pxt_fwd = 2 if prec == "fp32" else 1
    if wgrad_rows is None:
        wgrad_rows = next((r for r in ((7, 4, 2, 1) if prec == "bf16" else (4, 2, 1)) if mb * -(-H // r) >= 128), 1)
    return dict(B=B, level=level, CH=64 * pxt_fwd, CH1=64 * pxt_dgrad, R=wgrad_rows, max_batch=mb, k=k, lr=n32(lr),
                momentum=n32(momentum), dampening=n32(dampening), wd=n32(weight_decay), nesterov=bool(nesterov),
                first_step=bool(first_step), world=world, prec=prec,
                plain_fc_fresh=(level < 3) if plain_fc_fresh is None else plain_fc_fresh)


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


def copy_of(master, kind, a=0, b=0, c=0):
    """The fp32 re-ordered copy of a flat fp32 master in layout ``kind``."""
    flat = master.detach().cpu().float().reshape(-1)
    out = torch.zeros(K.shadow_dst_numel(kind, flat.numel()))
    out[torch.from_numpy(K.shadow_index(kind, flat.numel(), a, b, c))] = flat
    return out


def entry_shadows_fp32(before):
    return {"w2t_f32": copy_of(before["w2"], K.SHADOW_F32_TAPT, C2, 9, C1),
            "wfc_frag32": copy_of(before["wfc"], K.SHADOW_F32_FCFRAG, HW, C2)}


def wgrad_nslot(W_, R_):
    """The pixel slots conv3x3_wgrad's MFMA chain runs over for R_ rows of width W_: roundup32(R roundup8(W))."""
    return (R_ * ((W_ + 7) & ~7) + 31) // 32 * 32


def nslot(R_):
    return wgrad_nslot(W, R_)


def wgrad_rows_of(dy, x, R_, dtype=torch.float64):
    """conv3x3_wgrad's slab rows [B * ceil(H / R)][Co * 9 * Ci + Co] in ``dtype`` for dy [B,H,W,Co]
    and x [B,H,W,Ci] of any geometry: row = image n, chunk c of R output rows - (dW OHWI, db) of
    those rows alone."""
    dy, x = dy.detach().cpu().to(dtype), x.detach().cpu().to(dtype)
    B, Hh, _, Co = dy.shape
    nw = Co * 9 * x.shape[3]
    nRC = -(-Hh // R_)
    sh = [R._shift(x, kh - 1, kw - 1) for kh in range(3) for kw in range(3)]
    rows = torch.zeros(B, nRC, nw + Co, dtype=dtype)
    for c in range(nRC):
        r0, r1 = c * R_, min(Hh, (c + 1) * R_)
        d = dy[:, r0:r1]
        dw = torch.stack([torch.einsum("nhwo,nhwi->noi", d, s[:, r0:r1]) for s in sh], 2)  # [B,Co,9,Ci]
        rows[:, c, :nw] = dw.reshape(B, -1)
        rows[:, c, nw:] = d.sum(dim=(1, 2))
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


def fold_terms(b, CH, HW_=HW):
    """(block, slot) of every partial summed into image b's logits (common.h xent_logit_idx), for
    images of HW_ pixels in blocks of CH."""
    p0 = b * HW_
    kb0, kb1 = p0 // CH, (p0 + HW_ - 1) // CH
    return [(kb0 + j, (0 if kb0 * CH == p0 else 1) if j == 0 else 0) for j in range(kb1 - kb0 + 1)]


def _xent(x, absum, G, labels, gscale):
    rl, p = R.xent_rows64(x, labels)
    _, dref = R.xent64(x, labels, gscale)
    bd, bl = K.xent_rows_bounds(x, absum, G, labels, gscale, p, rl)
    return dref, rl, bd, bl


def check_step(obs, before, x_u8, labels, B, plan):
    """{stage: (largest error / bound, index of the worst element)} for the stages present in
    ``obs`` (see the module docstring; plan["prec"] picks the table).  ``obs``: CPU tensors by
    name - the entry shadows, a1, a2, fc_part, dlogits, loss_rows, loss_hist (+ loss_hist_before),
    dz2, dz1, w2slab, w1slab, grads {name: tensor}, params_after {name: tensor}, momentum_before /
    momentum_after {name: tensor}.  ``before``: the fp32 masters before the step; ``x_u8``
    [B,28,28] uint8 and ``labels`` [B]: the step's batch, gathered by the caller from the
    sampler's index list."""
    res = {}
    x_u8, labels = x_u8.detach().cpu(), labels.detach().cpu().long()
    assert x_u8.shape == (B, H, W) and labels.shape == (B,)
    P = {k: before[k].detach().cpu().float().reshape(SHAPES[k]) for k in PARAMS}
    f32 = plan.get("prec", "bf16") == "fp32"
    # the operands: the bf16 shadows' values, or the masters themselves
    w2o, wfco = (P["w2"], P["wfc"]) if f32 else (bf(P["w2"]), bf(P["wfc"]))
    stored = (lambda ref, E: E) if f32 else bf16_store_bound  # fp32 stores do not round

    def ab(n, A):
        return acc_bound(n, A, f32)

    scale = n32(1.0 / plan["world"])
    gscale = n32(np.float32(1.0) / np.float32(B))

    # ---- shadows at step entry
    if f32:
        want = entry_shadows_fp32(P)
        sh = [bitwise(obs[k].reshape(-1), want[k]) for k in ("w2t_f32", "wfc_frag32") if k in obs]
    else:
        want = entry_shadows(P)
        sh = [bitwise(obs[k].reshape(-1), want[k]) for k in ("w2_bf16", "w2t_bf16", "wfc_frag") if k in obs]
        if plan["plain_fc_fresh"] and "wfc_bf16" in obs:
            sh.append(bitwise(obs["wfc_bf16"].reshape(-1), want["wfc_bf16"]))
    if sh:
        res["shadows"] = max(sh, key=lambda t: t[0])

    # ---- forward
    a2 = obs["a2"].reshape(-1)[:B * HW * C2].view(B, H, W, C2)
    x01 = f64(x_u8) / 255.0
    A1 = R.conv3x3_64(x01.unsqueeze(-1), f64(P["w1"]).abs(), f64(P["b1"]).abs())
    if f32:
        # a1 is never stored: the float64 conv1, its bound e_a1 carried into a2, the w2 slab rows
        # and (through the recomputed mask's ambiguous set) the carried dz1
        assert "a1" not in obs and "dz1" not in obs, "the fp32 step stores neither a1 nor dz1"
        pre = R.conv1_64(x_u8, P["w1"].reshape(C1, 9), P["b1"], relu=False)
        a1, e_a1 = torch.relu(pre), ab(11, A1)
        amb = pre.abs() <= e_a1
        share = amb.double().mean().item()
        assert share <= AMBIG_CAP, f"{int(amb.sum())} of {amb.numel()} conv1 masks are ambiguous: more than {AMBIG_CAP}"
        keep1 = pre > 0
        ref = R.conv3x3_64(a1, w2o, P["b2"], True)
        A = R.conv3x3_64(a1 + e_a1, w2o.abs(), P["b2"].abs())
        res["a2"] = worst(a2, ref, ab(9 * C1 + 1, A) + R.conv3x3_64(e_a1, w2o.abs()))
    else:
        a1 = obs["a1"].reshape(-1)[:B * HW * C1].view(B, H, W, C1) if "a1" in obs else None
        if a1 is not None:
            ref = R.conv1_64(x_u8, P["w1"].reshape(C1, 9), P["b1"])
            res["a1"] = worst(a1, ref, bf16_store_bound(ref, acc_bound(11, A1)))
        else:  # (a chain that never stores a1: the float64 conv1, rounded as the kernel stores it)
            a1 = bf(R.conv1_64(x_u8, P["w1"].reshape(C1, 9), P["b1"]))
        ref = R.conv3x3_64(a1, w2o, P["b2"], True)
        A = R.conv3x3_64(a1.abs(), w2o.abs(), P["b2"].abs())
        res["a2"] = worst(a2, ref, bf16_store_bound(ref, acc_bound(9 * C1 + 1, A)))
        keep1 = f64(a1) > 0

    # ---- logits, cross-entropy
    xe = R.fc64(a2, wfco, P["bfc"])
    Ae = R.fc64(a2.abs(), wfco.abs(), P["bfc"].abs())
    # (xent_rows_bounds takes e_l = 2 G u A: the exact-fp32 3 n u A is G = 1.5 n)
    dl_ref, rl_ref, bd, bl = _xent(xe, Ae, (HW * C2 + HW // 16 + 1) * (1.5 if f32 else 1), labels, gscale)
    if "fc_part" in obs:
        CH = plan["CH"]
        nblk = -(-B * HW // CH)
        part = obs["fc_part"].reshape(-1)[:nblk * 2 * NO].view(nblk, 2, NO)
        pref = R.fc_block_partials64(a2, wfco, CH)
        pA = R.fc_block_partials64(a2.abs(), wfco.abs(), CH)
        res["fc_part"] = worst(part, pref, ab(16 + 4 + CH // 4 if f32 else 64 * CH + CH // 4, pA))
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
    ref, _, _ = R.fc_bwd64(dl64, a2, wfco, 1.0, True)
    A, _, _ = R.fc_bwd64(dl64.abs(), a2, wfco.abs(), 1.0, True)
    E = ab(NO, A)
    if e_d is not None:
        E = E + R.fc_bwd64(e_d, a2, wfco.abs(), 1.0, True)[0]
    res["dz2"] = worst(dz2, ref, stored(ref, E), exact_zero=~keep2)
    _, gw, gb = R.fc_bwd64(dl64, a2, wfco, scale, False)
    _, Aw, Ab = R.fc_bwd64(dl64.abs(), a2.abs(), wfco, scale, False)
    Ew, Eb = ab(B + 2, Aw), ab(B + 2, Ab)
    if e_d is not None:
        _, cw, cb = R.fc_bwd64(e_d, a2.abs(), wfco, scale, False)
        Ew, Eb = Ew + cw, Eb + cb
    gref = {"wfc": (gw, Ew), "bfc": (gb, Eb)}

    # ---- conv backward
    CH1 = plan["CH1"]
    if f32:
        # dz1 stays in registers (level >= 1) and is fp32: no store term.  An ambiguous mask may go
        # either way, so there the bound is the whole unmasked value besides its accumulation bound
        dun = R.conv3x3_dgrad64(dz2, w2o)
        Ea = ab(9 * C2, R.conv3x3_dgrad64(dz2.abs(), w2o.abs()))
        d1 = dun * keep1
        E1 = torch.where(amb, dun.abs() + Ea, Ea * keep1)
        r1 = w1_rows_of(d1, x01, CH1)
        E1r = ab(CH1 + 9, w1_rows_of(d1.abs() + E1, x01, CH1)) + w1_rows_of(E1, x01, CH1)
        r2 = wgrad_rows_of(dz2, a1, plan["R"])
        c2 = wgrad_rows_of(dz2.abs(), e_a1, plan["R"])
        c2[:, N_W2:] = 0.0  # (the bias columns do not read a1)
        E2r = ab(nslot(plan["R"]), wgrad_rows_of(dz2.abs(), a1 + e_a1, plan["R"])) + c2
    else:
        d1 = R.conv3x3_dgrad64(dz2, w2o) * keep1
        E1 = bf16_store_bound(d1, acc_bound(9 * C2, R.conv3x3_dgrad64(dz2.abs(), w2o.abs()) * keep1))
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
    grads = obs.get("grads", {})
    GR = K.reduce_groups([r2.shape[0], r1.shape[0]])
    for name, rows, Er, nw, gw_, gb_ in (("w2slab", r2, E2r, N_W2, "w2", "b2"), ("w1slab", r1, E1r, C1 * 9, "w1", "b1")):
        tot = Er.sum(0)
        if name in obs:
            slab = obs[name].reshape(-1)[:rows.numel()].view(rows.shape)
            res[name] = worst(slab, rows, Er)
            tot = tot + K.reduce_bound(f64(slab), scale)
            if f32 and torch.isfinite(slab).all():
                # the reduced gradients are the float32 replay of the stored rows, bit for bit
                red = torch.from_numpy(K.replay_finish(K.replay_reduce(slab.float().numpy(), GR), scale))
                for k_, part_ in ((gw_, red[:nw]), (gb_, red[nw:])):
                    if k_ in grads:
                        res[f"replay_{k_}"] = bitwise(grads[k_].reshape(-1).float(), part_)
        else:
            tot = tot + K.reduce_bound(rows.abs() + Er, scale)
        g = scale * rows.sum(0)
        gref[gw_] = (g[:nw].reshape(SHAPES[gw_]), scale * tot[:nw].reshape(SHAPES[gw_]))
        gref[gb_] = (g[nw:], scale * tot[nw:])

    # ---- the gradients in the flat buffer, the optimizer
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
                 drop_image=None, gscale=None, drop_w2_row=None, hist_slot=None, **fp32_errors):
    """An fp32 / bf16 model of the engine's stage outputs for the batch (x_u8 [B,28,28], labels
    [B]) from the masters ``before``: the ``obs`` of :func:`check_step`, every stage present
    (level 0 with the gradients stored and the optimizer applied).

    Planted wiring errors (tests/test_engine_step_bounds_cpu.py): ``drop_image`` - an image left
    out of every gradient sum; ``gscale`` - another cross-entropy scale than 1 / B;
    ``drop_w2_row`` - a conv2 slab row the reduction skips; ``hist_slot`` - the loss written to
    another slot than plan["k"]."""
    plan = plan or make_plan(B)
    if plan.get("prec", "bf16") == "fp32":
        return _emulate_fp32(before, x_u8, labels, B, plan, momentum_before, loss_hist_before, drop_image, gscale,
                             drop_w2_row, hist_slot, **fp32_errors)
    assert not fp32_errors, sorted(fp32_errors)
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


def _emulate_fp32(before, x_u8, labels, B, plan, momentum_before=None, loss_hist_before=None, drop_image=None,
                  gscale=None, drop_w2_row=None, hist_slot=None, bf16_w2=False, bf16_wfc=False, w2t=None,
                  zero_w2_half=None, borrow_w2_half=None, swap_w1_halves=None, flip_mask=None):
    """emulate_step for plan["prec"] == "fp32": torch's float32 operators on the masters, no bf16
    rounding anywhere, a1 and dz1 left out of ``obs`` (the step never stores them); fc_part,
    dlogits and loss_rows are all present - :func:`stored_on` keeps a chain's set.

    Planted errors besides emulate_step's: ``bf16_w2`` / ``bf16_wfc`` - the weight rounded to
    bf16 wherever a kernel reads it (a bf16 build wired into the fp32 chain; the copies keep the
    master's bits); ``w2t`` - "plain": w2t_f32 left in the master's OHWI order, or a masters dict:
    w2t_f32 derived from those (a step stale) - the dgrad reads what the copy holds;
    ``zero_w2_half`` / ``borrow_w2_half`` - the ci 16..31 columns of that w2slab row zeroed / taken
    from the row after it (the one before the last row); ``swap_w1_halves`` - the two conv1-channel
    halves of that w1slab row exchanged; ``flip_mask`` - the recomputed conv1 ReLU mask of one
    element (b, h, w, c) inverted in the dgrad role."""
    P = {k: before[k].detach().cpu().float().reshape(SHAPES[k]) for k in PARAMS}
    x_u8, labels = x_u8.detach().cpu(), labels.detach().cpu().long()
    x = x_u8.float() / 255.0
    obs = dict(entry_shadows_fp32(P))
    if isinstance(w2t, dict):
        obs["w2t_f32"] = entry_shadows_fp32(w2t)["w2t_f32"]
    elif w2t == "plain":
        obs["w2t_f32"] = P["w2"].reshape(-1).clone()
    else:
        assert w2t is None, w2t
    w2, wfc = (R.bf16r(P["w2"]) if bf16_w2 else P["w2"]), (R.bf16r(P["wfc"]) if bf16_wfc else P["wfc"])
    # the data gradient's operand is the [tap][ci][co] copy
    w2d = obs["w2t_f32"][torch.from_numpy(K.shadow_index(K.SHADOW_F32_TAPT, N_W2, C2, 9, C1))].view(SHAPES["w2"])
    w2d = R.bf16r(w2d) if bf16_w2 else w2d
    a1 = R.conv1_relu(x, P["w1"], P["b1"])
    a2 = R.conv3x3(a1, w2, P["b2"], relu=True)
    obs["a2"] = a2
    CH = plan["CH"]
    nblk = -(-B * HW // CH)
    per_px = torch.einsum("bpc,opc->bpo", a2.reshape(B, HW, C2), wfc)
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
    dz2 = (dl @ wfc.reshape(NO, -1)).view_as(a2) * (a2 > 0)
    obs["dz2"] = dz2
    mask1 = a1 > 0
    if flip_mask is not None:
        mask1[tuple(flip_mask)] = ~mask1[tuple(flip_mask)]
    dz1 = R.conv3x3_dgrad(dz2, w2d) * mask1
    live = torch.ones(B, dtype=torch.bool)
    if drop_image is not None:
        live[drop_image] = False
    s = np.float32(1.0 / plan["world"])
    g = {"wfc": ((dl[live].t() @ a2.reshape(B, -1)[live]) * s).view(SHAPES["wfc"]), "bfc": dl[live].sum(0) * s}
    nRC = -(-H // plan["R"])
    w2slab = wgrad_rows_of(dz2, a1, plan["R"], torch.float32)
    w1slab = w1_rows_of(dz1, x, plan["CH1"], torch.float32)
    hi2 = (torch.arange(N_W2) % C1 >= 16).nonzero().reshape(-1)  # the ci 16..31 columns: the second block's
    if zero_w2_half is not None:
        w2slab[zero_w2_half, hi2] = 0.0
    if borrow_w2_half is not None:
        other = borrow_w2_half + 1 if borrow_w2_half + 1 < w2slab.shape[0] else borrow_w2_half - 1
        w2slab[borrow_w2_half, hi2] = w2slab[other, hi2]
    if swap_w1_halves is not None:
        r = w1slab[swap_w1_halves].clone()
        w1slab[swap_w1_halves] = torch.cat([r[144:288], r[:144], r[304:320], r[288:304]])
    obs["w2slab"], obs["w1slab"] = w2slab, w1slab
    use2 = live.repeat_interleave(nRC)
    if drop_w2_row is not None:
        use2[drop_w2_row] = False
    r1 = w1slab if drop_image is None else w1_rows_of(dz1 * live.view(B, 1, 1, 1), x, plan["CH1"], torch.float32)
    GR = K.reduce_groups([w2slab.shape[0], w1slab.shape[0]])
    # (a skipped row adds +0.0f in its place: the other rows keep their groups)
    red2 = torch.from_numpy(K.replay_finish(K.replay_reduce((w2slab * use2.view(-1, 1)).numpy(), GR), s))
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


def stored_on(obs, level):
    """``obs`` without what the fp32 chain ``level`` keeps on chip: level 1 the dL rows and the row
    losses (fc_bwd's prologue), level 3 the partial logits (handed over as granules)."""
    drop = ("fc_part",) if level >= 3 else ("dlogits", "loss_rows")
    return {k: v for k, v in obs.items() if k not in drop}


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
