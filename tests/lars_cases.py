"""The LARS layouts at the sizes a whole model reaches (tests/test_lars_scale_gpu.py runs the
kernels on them, tests/test_lars_scale_cpu.py checks that they reach every loop they are meant
for and that wrong kernels would be caught on them).  A helper module, not a test module.

``WIDE`` - one flat buffer, every tensor on a 64-element boundary, in this order:

* 130 items + 9 elements: its first items are full 4096-element pieces, taken by blocks 0, 1, ...
  of seg_sqnorm_kernel's 2048-block grid, and its 131 partials make lane j of the per-tensor
  finish loop (``for (k = lane; k < ni; k += 64)``) run up to three trips;
* exactly 64 items (one partial per lane, the last lane included) and 65 items + 1 element (lanes
  0 and 1 take a second partial, the last of them from a one-element item);
* 1900 short tensors of 1 .. 65 elements, in a cycle (every n % 4, the 63 / 64 / 65 edges): they
  push n_items past LARS_MAX_BLOCKS, so the item loop (``for (e = blockIdx.x; ...; e += gridDim.x)``)
  takes a second item in 626 blocks - the second ``__syncthreads()`` and the last-arrival ticket
  at the full grid; the items 2048 .. 2160 are short tensors, so blocks 0 .. 112 run a full item
  and then a short one (the clamp-and-zero loads after a full item); and they push n_seg + 1 past
  3 x 256, so lars_kernel's LDS table fill (``for (i = threadIdx.x; i <= n_seg; i += blockDim.x)``)
  makes up to eight trips;
* one last tensor of 4 * 256 * 2048 + 3 * 1024 + 5 elements: longer than a whole flat_stream pass
  at the 2048-block grid cap, so every quad of the second grid-stride pass lies in this tensor
  while the quad the same thread took in the first pass lies in another one (only LarsRule
  looks a quad's tensor up, per quad).

``wide_tail()`` is WIDE in a buffer of N + 3 elements: three elements of null-segment padding
that go through flat_stream's scalar tail.

``MAX_SEGS`` - LARS_MAX_SEGS one-chunk tensors of 1 .. 64 elements: the wave loop of the finish
over 4095 tensors, 2047 blocks with two items each, the 32 KiB LDS table whose entry 4095 is the
null segment.  ``too_many_tables()`` is the same for 4096 tensors, which lars_plan must refuse.

Inputs (``Layout.inputs``): weight scales 0.1 / 1 / 10 and gradient scales 1 .. 1e-3 by tensor
as tests/test_lars_cpu.py ``make_inputs``; WIDE's last tensor has weights of 0.03 and gradients
of 3, which puts its ratio two orders of magnitude from the ratios of the tensors that own its
quads' first-pass aliases.  Every seventh tensor is excluded (adapt 0, wd 0), one tensor has
all-zero weights and one an all-zero gradient.  What a seed returns is shared: do not write it.
"""
import functools

import numpy as np
import torch

from ddp_amd.ops import kernel_bounds as kb
from ddp_amd.ops.lars import lars_layout

ITEM, CHUNK = kb.LARS_ITEM, kb.LARS_CHUNK
WD, TC, EPS, LR, MOM, COEF = 0.1, 0.02, 1e-8, 0.05, 0.9, 0.37
FLAT_THREADS, FLAT_MAX_BLOCKS = 256, 2048  # csrc/kernels/flat_step.h


def flat_grid(n):
    """flat_grid (flat_step.h): the blocks of a flat_stream launch over n elements."""
    return int(min(max(((n >> 2) + FLAT_THREADS - 1) // FLAT_THREADS, 1), FLAT_MAX_BLOCKS))


def flat_passes(n):
    """Grid-stride passes of flat_stream over n elements."""
    per = flat_grid(n) * FLAT_THREADS
    return ((n >> 2) + per - 1) // per


class Layout:
    def __init__(self, name, lens, zero_w=None, zero_g=None, scales=None, tail=0, excluded=None):
        self.name, self.lens, self.tail = name, [int(m) for m in lens], tail
        self.n_seg = len(self.lens)
        spans = [-(-m // CHUNK) * CHUNK for m in self.lens]
        self.begins = [int(b) for b in np.cumsum([0] + spans[:-1])]
        self.N = self.begins[-1] + spans[-1]  # the tensors and their padding
        self.n = self.N + tail                # the flat buffer
        self.segs = list(zip(self.begins, self.lens))
        self.excluded = [i % 7 == 3 for i in range(self.n_seg)] if excluded is None else list(excluded)
        self.zero_w, self.zero_g = zero_w, zero_g
        assert zero_w is None or not (self.excluded[zero_w] or self.excluded[zero_g])
        self.wds = [0.0 if e else WD for e in self.excluded]
        self.adapts = [not e for e in self.excluded]
        self.scales = {} if scales is None else scales  # tensor -> (weight scale, gradient scale)
        self.seg_items = np.array([kb.lars_items(m) for m in self.lens])
        self.item0 = np.concatenate([[0], np.cumsum(self.seg_items)[:-1]])
        self.n_items = int(self.seg_items.sum())
        self.item_seg = np.repeat(np.arange(self.n_seg), self.seg_items)
        k = np.arange(self.n_items) - self.item0[self.item_seg]
        self.item_begin = np.array(self.begins)[self.item_seg] + k * ITEM
        self.item_len = np.minimum(ITEM, np.array(self.lens)[self.item_seg] - k * ITEM)
        self.seg_of = np.full(self.n, self.n_seg, dtype=np.int64)  # per element; n_seg: padding
        for s, (b, m) in enumerate(self.segs):
            self.seg_of[b:b + m] = s
        self.inside = self.seg_of < self.n_seg

    def tables(self):
        """(segs, items, cmap) of lars_layout for the buffer of n elements."""
        return lars_layout(self.begins, self.lens, self.n, self.wds, self.adapts)

    def scale_of(self, i):
        return self.scales.get(i, (10.0 ** (i % 3 - 1), 10.0 ** -(i % 4)))

    def make_inputs(self, seed):
        """Flat float32 (w, g, m) of n elements: zero padding between the tensors, 0.5 in the
        ``tail`` elements behind them (null-segment padding: plain SGD there)."""
        gen = torch.Generator().manual_seed(seed)
        sw = np.zeros(self.n, dtype=np.float32)
        sg = np.zeros(self.n, dtype=np.float32)
        for i, (b, m) in enumerate(self.segs):
            sw[b:b + m], sg[b:b + m] = self.scale_of(i)
        if self.zero_w is not None:
            b, m = self.segs[self.zero_w]
            sw[b:b + m] = 0
            b, m = self.segs[self.zero_g]
            sg[b:b + m] = 0
        w = torch.randn(self.n, generator=gen) * torch.from_numpy(sw)
        g = torch.randn(self.n, generator=gen) * torch.from_numpy(sg)
        mm = torch.randn(self.n, generator=gen) * torch.from_numpy(sg) * 0.05
        for x in (w, g, mm):
            x[self.N:] = 0.5
        return w, g, mm

    @functools.lru_cache(maxsize=None)
    def inputs(self, seed=1):
        """``make_inputs(seed)``, made once and shared."""
        return self.make_inputs(seed)

    def segs_ref(self):
        """(segs, wds, adapts) for kernel_bounds.lars_reference: the tail as one more tensor
        without decay or ratio."""
        t = bool(self.tail)
        return self.segs + [(self.N, self.tail)] * t, self.wds + [0.0] * t, self.adapts + [False] * t

    def item_rows(self, x):
        """[n_items][ITEM] float32: every work item's elements, +0.0f at and past its len."""
        x = np.asarray(x, dtype=np.float32)
        col = np.arange(ITEM)
        idx = np.minimum(self.item_begin[:, None] + col, self.n - 1)
        return np.where(col < self.item_len[:, None], x[idx], np.float32(0))

    def finish(self, part):
        """[n_items] partials -> [n_seg] sums, kernel_bounds.replay_seg_finish per tensor."""
        return np.array([kb.replay_seg_finish(part[e:e + k]) for e, k in zip(self.item0, self.seg_items)],
                        dtype=np.float32)

    def replay(self, x):
        """(partials [n_items], sums [n_seg]) of the flat buffer x in seg_sqnorm_kernel's order."""
        part = kb.replay_item_partials(self.item_rows(x))
        return part, self.finish(part)

    @functools.lru_cache(maxsize=None)
    def replayed(self, which, seed):
        """``replay`` of inputs(seed)[which] (0: w, 1: g), computed once."""
        return self.replay(self.inputs(seed)[which].numpy())

    def trust(self, sw, sg, coef=None):
        """float32 [n_seg, 4] {ratio, wd, wn, gn} from the sums of squares (trust_ratio32)."""
        out = np.zeros((self.n_seg, 4), dtype=np.float32)
        for i in range(self.n_seg):
            wn, gn, ratio = kb.trust_ratio32(sw[i], sg[i], self.wds[i], TC, EPS, self.adapts[i], coef)
            out[i] = (ratio, self.wds[i], wn, gn)
        return out

    def ratios64(self, w, g, coef=None):
        """The float64 ratio of every tensor (1 for an excluded or degenerate one)."""
        w, g = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (w, g))
        out = np.ones(self.n_seg)
        for i, (b, m) in enumerate(self.segs):
            wn, gn = np.sqrt((w[b:b + m] ** 2).sum()), np.sqrt((g[b:b + m] ** 2).sum())
            gn = gn if coef is None else gn * float(np.float32(coef))
            if self.adapts[i] and wn > 0 and gn > 0:
                wd = float(np.float32(self.wds[i]))
                out[i] = float(np.float32(TC)) * wn / (wd * wn + gn + float(np.float32(EPS)))
        return out


BIG, SIXTY_FOUR, SIXTY_FIVE, SHORT0, N_SHORT = 0, 1, 2, 3, 1900
LAST = SHORT0 + N_SHORT
WIDE_LENS = ([130 * ITEM + 9, 64 * ITEM, 65 * ITEM + 1] + [1 + i % 65 for i in range(N_SHORT)]
             + [4 * FLAT_THREADS * FLAT_MAX_BLOCKS + 3 * 4 * FLAT_THREADS + 5])
_WIDE = dict(lens=WIDE_LENS, zero_w=300, zero_g=1000, scales={LAST: (0.03, 3.0)})
WIDE = Layout("wide", **_WIDE)
MAX_SEGS = Layout("max_segs", [1 + i % 64 for i in range(kb.LARS_MAX_SEGS)], zero_w=300, zero_g=4001)
LAYOUTS = {"wide": WIDE, "max_segs": MAX_SEGS}


@functools.lru_cache(maxsize=None)
def wide_tail():
    return Layout("wide_tail", tail=3, **_WIDE)


def too_many_tables():
    """(segs, items, cmap, n) of LARS_MAX_SEGS + 1 one-chunk tensors, written out by hand
    (lars_layout refuses them itself): what lars_plan must refuse."""
    k = kb.LARS_MAX_SEGS + 1
    idx = np.arange(k, dtype=np.int32)
    lens = 1 + idx % 64
    segs = np.zeros((k, 8), dtype=np.int32)
    segs[:, 0], segs[:, 1], segs[:, 2], segs[:, 3], segs[:, 5] = idx, lens, idx, 1, 1
    items = np.stack([idx, lens, idx, np.zeros_like(idx)], axis=1).astype(np.int32)
    return torch.from_numpy(segs), torch.from_numpy(items), torch.from_numpy(idx.astype(np.int16)), k * CHUNK
