"""The whole-model LARS cases (tests/lars_cases.py) on the CPU: they reach the loops they exist
for, and a kernel that got one of those loops wrong would miss the checks of
tests/test_lars_scale_gpu.py on these very inputs.

* coverage - the item grid-stride loop of seg_sqnorm_kernel (n_items past the 2048-block grid, a
  full item followed by a short one in the same block), its per-tensor finish loop (64 items, 65
  items + 1 element, 130 items + 9 elements), lars_kernel's LDS table fill (n_seg + 1 past three
  trips of 256 threads; 4096 entries), flat_stream's grid cap and second pass under LarsRule (a
  second-pass quad in another tensor than its first-pass alias, with a ratio that differs from
  the alias's by more than 100 x trust_ratio_bound);
* wrong variants of the replay, (a) .. (d), each a way one of these loops can fail: they differ
  from kernel_bounds.replay_seg_sqnorm in bits, and (a) .. (c) move a ratio out of
  trust_ratio_bound;
* wrong variants of the update rule, (e) and (f): each leaves elements outside the bounds of
  kernel_bounds.lars_reference, while the right rule, written out independently, has none.
"""
import numpy as np
import pytest

from ddp_amd.ops import kernel_bounds as kb
from lars_cases import (BIG, COEF, EPS, FLAT_MAX_BLOCKS, FLAT_THREADS, ITEM, LAST, LR, MAX_SEGS, MOM, N_SHORT, SHORT0,
                        SIXTY_FIVE, SIXTY_FOUR, TC, WIDE, flat_grid, flat_passes, too_many_tables, wide_tail)

GRID = kb.LARS_MAX_BLOCKS
STRIDE = FLAT_THREADS * FLAT_MAX_BLOCKS  # quads of one flat_stream pass at the grid cap


def alias_pairs(L):
    """(tensor of every second-pass quad, tensor of the quad the same thread took in the first
    pass), through the chunk map as LarsRule reads it."""
    cmap = L.tables()[2].numpy().astype(np.int64)
    q = np.arange(STRIDE, L.n >> 2)
    return cmap[(q << 2) >> 6], cmap[((q - STRIDE) << 2) >> 6]


# ------------------------------------------------------------------------------ coverage
def test_wide_reaches_every_loop():
    L = WIDE
    assert kb.LARS_ITEM == ITEM == 4096 and kb.LARS_MAX_BLOCKS == 2048 and kb.LARS_MAX_SEGS == 4095
    assert all(b % 64 == 0 for b in L.begins) and L.N % 64 == 0
    segs, items, cmap = L.tables()
    assert segs.shape == (L.n_seg, 8) and items.shape == (L.n_items, 4) and cmap.shape == (L.N // 64,)
    assert np.array_equal(items[:, 0].numpy() * 64, L.item_begin) and np.array_equal(items[:, 1].numpy(), L.item_len)
    assert np.array_equal(items[:, 2].numpy(), L.item_seg) and np.array_equal(segs[:, 2].numpy(), L.item0)
    # the per-tensor finish loop: one partial in every lane; a second one from a one-element
    # item; three trips with a ragged last item
    assert L.seg_items[SIXTY_FOUR] == 64 and L.lens[SIXTY_FOUR] == 64 * ITEM
    assert L.seg_items[SIXTY_FIVE] == 66 and L.lens[SIXTY_FIVE] == 65 * ITEM + 1
    assert L.seg_items[BIG] >= 130 and 0 < L.lens[BIG] % ITEM < ITEM and L.lens[BIG] % 4
    assert L.seg_items[LAST] > 8 * 64 and L.lens[LAST] % ITEM % 4
    # the item loop: a second item in at least 32 blocks, a full item then a short one
    assert L.n_items - GRID >= 32
    pairs = [b for b in range(L.n_items - GRID) if L.item_len[b] == ITEM and L.item_len[b + GRID] < 64 + 2]
    assert len(pairs) >= 32 and pairs[:32] == list(range(32))
    assert all(L.item_seg[b] == BIG and SHORT0 <= L.item_seg[b + GRID] < LAST for b in pairs[:32])
    assert {L.item_len[b + GRID] % 4 for b in pairs} == {0, 1, 2, 3}
    assert {63, 64, 65} <= {L.item_len[b + GRID] for b in pairs}
    assert any(L.item_len[b] == ITEM and L.item_len[b + GRID] == ITEM for b in range(L.n_items - GRID))
    short = L.lens[SHORT0:LAST]
    assert len(short) == N_SHORT and set(short) == set(range(1, 66))
    # the LDS table fill: more than three trips
    assert L.n_seg + 1 > 3 * 256
    # flat_stream: the grid cap, a second pass, and its quads in another tensor than their aliases
    assert flat_grid(L.n) == FLAT_MAX_BLOCKS and flat_passes(L.n) == 2
    assert L.lens[LAST] > 4 * STRIDE + 2 * 4 * FLAT_THREADS and L.n % 4 == 0
    own, alias = alias_pairs(L)
    assert (own == LAST).all(), "every second-pass quad lies in the last tensor"
    assert (alias != own).mean() > 0.99 and len(set(alias.tolist())) >= N_SHORT
    T = wide_tail()
    assert T.n == L.n + 3 and T.n % 4 == 3 and T.tables()[2].shape == (L.N // 64 + 1,)
    assert T.tables()[2][-1].item() == T.n_seg and flat_passes(T.n) == 2


def test_max_segs_reaches_every_loop():
    L = MAX_SEGS
    assert L.n_seg == kb.LARS_MAX_SEGS == L.n_items and L.n == 262080 and set(L.lens) == set(range(1, 65))
    assert all(k == 1 for k in L.seg_items)
    assert L.n_items - GRID == GRID - 1, "2047 blocks with two items each"
    assert 8 * (L.n_seg + 1) == 32 * 1024, "the 32 KiB table"
    assert L.tables()[0].shape == (4095, 8)
    segs, items, cmap, n = too_many_tables()
    assert segs.shape == (4096, 8) and items.shape == (4096, 4) and cmap.shape == (4096,) and n == 4096 * 64
    good = L.tables()  # the hand-written tables are lars_layout's but for the count (and wd / adapt)
    assert np.array_equal(segs[:4095, :4].numpy(), good[0][:, :4].numpy())
    assert np.array_equal(items[:4095].numpy(), good[1].numpy()) and np.array_equal(cmap[:4095].numpy(), good[2].numpy())


@pytest.mark.parametrize("name", ["wide", "wide_tail", "max_segs"])
def test_inputs_have_the_special_tensors(name):
    L = {"wide": WIDE, "wide_tail": wide_tail(), "max_segs": MAX_SEGS}[name]
    w, g, m = (x.numpy() for x in L.inputs(1))
    assert w.dtype == np.float32 and w.shape == (L.n,)
    assert not w[:L.N][~L.inside[:L.N]].any() and not g[:L.N][~L.inside[:L.N]].any() and not m[:L.N][~L.inside[:L.N]].any()
    b, k = L.segs[L.zero_w]
    assert not w[b:b + k].any() and g[b:b + k].all()
    b, k = L.segs[L.zero_g]
    assert not g[b:b + k].any() and w[b:b + k].all()
    ex = [i for i, e in enumerate(L.excluded) if e]
    assert len(ex) > L.n_seg // 8 and min(ex) < 256 <= max(ex) and sum(i >= 256 for i in ex) > 100
    assert all(L.wds[i] == 0.0 and not L.adapts[i] for i in ex)
    wn = np.array([np.abs(w[b:b + k]).max() for b, k in L.segs if k >= 16])
    gn = np.array([np.abs(g[b:b + k]).max() for b, k in L.segs if k >= 16])
    assert wn[wn > 0].max() / wn[wn > 0].min() > 30 and gn[gn > 0].max() / gn[gn > 0].min() > 300
    again = L.make_inputs(1)
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(L.inputs(1), again)), "deterministic"
    assert not np.array_equal(L.inputs(2)[1].numpy(), g)


@pytest.mark.parametrize("seed,coef", [(1, None), (1, COEF), (2, None)])
def test_ratios_are_separated(seed, coef):
    """Every adapted, non-degenerate tensor's float64 ratio differs from 1 by more than 100 x its
    bound, and the ratio of a tensor with second-pass quads differs as much from the ratio of
    every tensor that owns one of their first-pass aliases: a kernel that leaves a ratio at 1, or
    takes the alias's, cannot stay inside the bounds."""
    for L in (WIDE, MAX_SEGS, wide_tail()):
        w, g = L.inputs(1)[0].numpy(), L.inputs(seed)[1].numpy()
        R = L.ratios64(w, g, coef)
        rho = np.array([kb.trust_ratio_bound(m, coef is not None) for m in L.lens])
        live = np.array(L.adapts)
        live[[L.zero_w, L.zero_g]] = False
        assert (R[~live] == 1.0).all()
        assert (np.abs(R[live] - 1.0) > 100 * rho[live] * R[live]).all()
        if flat_passes(L.n) > 1:
            own, alias = alias_pairs(L)
            R1 = np.append(R, 1.0)  # the null segment
            for s, a in {(int(s), int(a)) for s, a in zip(own, alias) if s != a and s < L.n_seg}:
                assert live[s] and abs(R1[s] - R1[a]) > 100 * rho[s] * R1[s], (s, a)


# ------------------------------------------------------------------------------ the replay
def test_the_replays_square_is_the_fma():
    """replay_item_partials squares with the float32 multiply; the kernel with fmaf(x, x, +0.0f).
    The same bits, subnormal squares, squares that underflow and -0.0f included."""
    gen = np.random.default_rng(0)
    x = (gen.standard_normal(ITEM * 8) * 10.0 ** gen.integers(-24, 3, ITEM * 8)).astype(np.float32)
    x[:4] = (-0.0, 0.0, 1e-23, -3e-20)
    fma = kb._fma32(x, np.zeros_like(x))
    assert np.array_equal((x * x).view(np.int32), fma.view(np.int32))
    assert (fma == 0).sum() > 100 and ((fma > 0) & (fma < 1.1754944e-38)).sum() > 100
    rows = x.reshape(8, ITEM)
    sq = fma.reshape(8, 4, 256, 4)
    s = ((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]))
    th = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    assert s.dtype == np.float32 and np.array_equal(kb.replay_item_partials(rows), kb._block_sum(th))


def pairwise(part):
    """(d): the item partials folded pairwise (neighbours, then pairs of those, ...; an odd one
    is carried) - for at most 64 partials that is the kernel's order, one partial per lane."""
    v = [np.float32(p) for p in part]
    while len(v) > 1:
        v = [np.float32(v[i] + v[i + 1]) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def wrong_sums(L, part, variant):
    part = part.copy()
    if variant == "a":    # the items past the grid are never summed
        part[GRID:] = 0
    elif variant == "c":  # a block's second item reports its first item's partial (stale LDS)
        part[GRID:] = part[:L.n_items - GRID].copy()
    if variant == "b":    # the finish stops after one trip: a tensor's first 64 partials only
        return np.array([kb.replay_seg_finish(part[e:e + min(k, 64)]) for e, k in zip(L.item0, L.seg_items)])
    if variant == "d":
        return np.array([pairwise(part[e:e + k]) for e, k in zip(L.item0, L.seg_items)])
    return L.finish(part)


def out_of_bound(L, sw, sg, R64):
    """Tensors whose fp32 ratio from the sums (sw, sg) lies outside trust_ratio_bound of R64."""
    r32 = L.trust(sw, sg)[:, 0].astype(np.float64)
    rho = np.array([kb.trust_ratio_bound(m) for m in L.lens])
    return np.flatnonzero(np.abs(r32 - R64) > rho * R64)


@pytest.mark.parametrize("name", ["wide", "max_segs"])
def test_replay_meets_the_ratio_bound_and_wrong_replays_do_not(name):
    L = {"wide": WIDE, "max_segs": MAX_SEGS}[name]
    w, g, _ = (x.numpy() for x in L.inputs(1))
    (pw, sw), (pg, sg) = L.replayed(0, 1), L.replayed(1, 1)
    for i in (0, 1, 2, L.n_seg - 1):  # the one-call replay of a tensor is the layout's
        b, k = L.segs[i]
        assert kb.replay_seg_sqnorm(w[b:b + k]) == sw[i] and kb.replay_seg_sqnorm(g[b:b + k]) == sg[i]
    R64 = L.ratios64(w, g)
    assert out_of_bound(L, sw, sg, R64).size == 0, "the replayed order is inside its own bound"
    many = L.seg_items > 64
    for variant in ("a", "b", "c", "d"):
        vw, vg = wrong_sums(L, pw, variant), wrong_sums(L, pg, variant)
        differ = (vw.view(np.int32) != sw.view(np.int32)) | (vg.view(np.int32) != sg.view(np.int32))
        if name == "max_segs" and variant in "bd":  # (one item per tensor: nothing to fold)
            assert not differ.any()
            continue
        assert differ.any(), variant
        if variant in "bd":
            assert not differ[~many].any() and differ[many].any()
        if variant != "d":
            out = out_of_bound(L, vw, vg, R64)
            assert out.size and set(out) <= set(np.flatnonzero(differ)), variant
            print(f"[lars scale mutant] {name} ({variant}): {int(differ.sum())} tensors differ in bits, "
                  f"{out.size} ratios outside the bound")


# ------------------------------------------------------------------------------ the update rule
def rule64(L, w, g, m, R64, variant=None):
    """(p, m) of a regular momentum step in float64, every element's {ratio, wd} looked up
    through the chunk map as LarsRule does, or wrongly: "e" - table entries from 256 on read as
    the null segment; "f" - a second-pass quad takes the tensor of its first-pass alias."""
    cmap = L.tables()[2].numpy().astype(np.int64)
    q = np.arange(L.n) >> 2
    if variant == "f":
        q = np.where(q >= STRIDE, q - STRIDE, q)
    s = cmap[(q << 2) >> 6]
    if variant == "e":
        s = np.where(s >= 256, L.n_seg, s)
    R = np.append(R64, 1.0)[s]
    wd = np.append(np.array(L.wds, dtype=np.float32).astype(np.float64), 0.0)[s]
    w, g, m = (x.astype(np.float64) for x in (w, g, m))
    buf = float(np.float32(MOM)) * m + (g + wd * w) * R
    return w - float(np.float32(LR)) * buf, buf


@pytest.mark.parametrize("name", ["wide", "max_segs"])
def test_wrong_table_lookups_miss_the_bounds(name):
    L = {"wide": WIDE, "max_segs": MAX_SEGS}[name]
    w, g, m = (x.numpy() for x in L.inputs(1))
    p64, m64, R64, bp, bm = kb.lars_reference(w, g, m, L.segs, L.wds, L.adapts, LR, MOM, 0.0, False, False, False,
                                              TC, EPS)
    assert p64.shape == (L.n,) == bp.shape, "every element is compared"
    p, buf = rule64(L, w, g, m, R64)
    assert (np.abs(p - p64) <= bp).all() and (np.abs(buf - m64) <= bm).all(), "the independent rule agrees"
    for variant in ("e", "f"):
        p, buf = rule64(L, w, g, m, R64, variant)
        out_p, out_m = np.abs(p - p64) > bp, np.abs(buf - m64) > bm
        if name == "max_segs" and variant == "f":  # (one pass: no alias)
            assert not out_p.any() and not out_m.any()
            continue
        assert out_p.any() and out_m.any(), variant
        where = L.seg_of[out_p]
        assert (where >= 256).all() if variant == "e" else (where == LAST).all()
        print(f"[lars scale mutant] {name} ({variant}): {int(out_p.sum())} elements of p outside, worst error / bound "
              f"{float((np.abs(p - p64)[out_p] / bp[out_p]).max()):.3g}")
