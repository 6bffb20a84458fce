"""The loopback all-reduce cases (tests/test_xgmi_loopback_gpu.py) and a CPU model of the
kernel's index plan (tests/test_xgmi_plan_cpu.py checks that the cases reach every path).

``paths`` replays, in plain Python, which thread of which block of which rank takes which
item of ``xgmi_allreduce_body`` (csrc/kernels/xgmi_body.h) by which path, from the mapping the
kernel documents:

* thread t of block b owns quad q0 = b * 256 + t of a slice (one-shot: of the bucket), then
  q0 + G, q0 + 2G, ... with G = 256 * blocks;
* two-shot slices are ``slice_len(n, N)`` elements (n / N rounded up to whole quads); rank r
  reduces elements [r * slice, r * slice + lim) with lim = min(slice, n - r * slice), which
  may be short or <= 0;
* the reduce-scatter walks the thread's full quads as (quad j, rank p) items, p fastest,
  BATCH = 8 items per batch; a partial last quad goes through element loads;
* the all-gather walks (quad j, rank p) items over every rank's slice the same way, skips
  items past the bucket's end, stores whole quads of a 4-aligned bucket as vectors and
  everything else element by element;
* the one-shot kernel publishes the bucket in whole quads (first quad preloaded, zero-padded
  tail), then sums two quads per trip and an odd one after.

It returns labels, not values: the GPU test holds the values.
"""
import functools
from collections import namedtuple

THREADS = 256
BATCH = 8
MAX_RANKS = 8
GRID_CAP = 256
GROUP_MAX_BLOCKS = 64
MAX_SHADOWS = 4


def slice_len(n, N):
    """xgmi_slice: elements per rank slice, n / N rounded up to whole quads."""
    return (((n + N - 1) // N) + 3) & ~3


def blocks(n, N, oneshot, cap=0):
    """xgmi_blocks, then the channel's cap (add_channel's ``blocks``; 0: none)."""
    quads = ((n if oneshot else slice_len(n, N)) + 3) // 4
    b = max(1, min((quads + THREADS - 1) // THREADS, GRID_CAP))
    return min(b, cap) if cap > 0 else b


def stage_floats(n, N, oneshot):
    """xgmi_stage_floats: one parity of a rank's stage buffer."""
    return (n + 3) & ~3 if oneshot else slice_len(n, N)


def _ceil_div(a, b):
    return (a + b - 1) // b


def paths(N, n, off, nblk, oneshot, publish):
    """Labels of every path some thread takes in one call of the channel (N ranks, bucket
    [off, off + n), nblk blocks per rank)."""
    out = set()
    G = THREADS * nblk
    if oneshot:
        nq, fq = (n + 3) // 4, n // 4
        for b in range(nblk):
            ok = [b * THREADS + t < fq for t in range(THREADS)]
            if any(ok) and not all(ok):
                out.add("os_first_ok_mixed")
        for q0 in range(G):
            q = q0
            while q < nq:  # publish
                if q == q0 and q0 < fq:
                    out.add("os_first_quad")
                elif q < fq:
                    out.add("os_second_stride_full")
                else:
                    out.add("os_padded_tail")
                q += G
            q, trips, done = q0, 0, []
            while q + G < nq:  # sum: two quads per trip
                done += [q, q + G]
                trips += 1
                q += 2 * G
            if trips:
                out.add("os_paired")
            if q < nq:
                done.append(q)
                if trips:
                    out.add("os_odd_remainder")
            for q in done:
                if off % 4:
                    out.add("os_off_unaligned")
                elif 4 * q + 3 < n:
                    out.add("os_vector")
                else:
                    out.add("os_scalar_finish")
        return out

    sl = slice_len(n, N)
    sq = sl // 4
    # ---- publish pass (the same on every rank)
    if publish:
        for p in range(N):
            lim = min(sl, n - p * sl)
            if lim <= 0 and N > 1:
                out.add("pub_peer_empty")
            for q0 in range(G):
                q = q0
                while 4 * q < lim:
                    out.add("pub_quad" if 4 * q + 3 < lim else "pub_elem")
                    q += G
    # ---- reduce-scatter (rank r's slice)
    for r in range(N):
        lim = min(sl, n - r * sl)
        if lim <= 0:
            out.add("rs_empty_slice")
        elif lim < sl:
            out.add("rs_short_slice")
        fq = lim // 4 if lim > 0 else 0
        nq = (lim + 3) // 4 if lim > 0 else 0
        for q0 in range(G):
            J = _ceil_div(fq - q0, G) if fq > q0 else 0
            items = J * N
            if J >= 1:
                out.add("rs_full_quad")
            if J >= 2:
                out.add("rs_grid_stride")
            if items > BATCH:
                out.add("rs_multi_batch")
            if any(b % N for b in range(BATCH, items, BATCH)):
                out.add("rs_batch_splits_sum")
            if q0 + J * G < nq:  # the partial last quad
                out.add("rs_tail_%d" % (lim % 4))
                if J == 0:
                    out.add("rs_tail_only_thread")
    # ---- all-gather (the same on every rank)
    for q0 in range(G):
        Jg = _ceil_div(sq - q0, G) if sq > q0 else 0
        items = Jg * N
        if items > BATCH:
            out.add("ag_load_pm_later")
        for i0 in range(0, items, BATCH):
            quads, ranks = set(), set()
            for i in range(i0, min(i0 + BATCH, items)):
                jj, pp = divmod(i, N)
                qq = pp * sq + q0 + jj * G
                if 4 * qq >= n:
                    out.add("ag_skip")
                    continue
                quads.add(jj)
                ranks.add(pp)
                if off % 4:
                    out.add("ag_off_%d" % (off % 4))
                elif 4 * qq + 3 < n:
                    out.add("ag_vector")
                else:
                    out.add("ag_scalar_finish")
            if len(quads) >= 2 and len(ranks) >= 2:
                out.add("ag_mixed_batch")
    return out


RS_LABELS = {"rs_full_quad", "rs_batch_splits_sum", "rs_grid_stride", "rs_multi_batch", "rs_tail_1", "rs_tail_2",
             "rs_tail_3", "rs_empty_slice", "rs_short_slice", "rs_tail_only_thread"}
AG_LABELS = {"ag_vector", "ag_scalar_finish", "ag_off_1", "ag_off_2", "ag_off_3", "ag_skip", "ag_mixed_batch",
             "ag_load_pm_later"}
PUB_LABELS = {"pub_quad", "pub_elem", "pub_peer_empty"}
OS_LABELS = {"os_first_ok_mixed", "os_first_quad", "os_second_stride_full", "os_padded_tail", "os_paired",
             "os_odd_remainder", "os_vector", "os_scalar_finish", "os_off_unaligned"}
CALL_LABELS = {"calls_both_parities"}
# with the fused SGD: the labels of the two-shot plan again, reached by a case that updates
# parameters (the select chain also picks the preloaded parameter / momentum quads)
SGD_LABELS = {"sgd:ag_mixed_batch", "sgd:ag_load_pm_later", "sgd:ag_vector", "sgd:ag_scalar_finish", "sgd:ag_off_1",
              "sgd:ag_off_2", "sgd:ag_off_3", "sgd:os_vector", "sgd:os_scalar_finish", "sgd:os_off_unaligned"}
ALL_LABELS = RS_LABELS | AG_LABELS | PUB_LABELS | OS_LABELS | CALL_LABELS | SGD_LABELS


def exempt(N):
    """Labels no bucket can reach at world size N.
    N = 1: no peer - a quad's rank sum is one item, the only slice holds the whole bucket (never
    empty, nothing to skip), a batch holds one rank.  N = 2, 4, 8 divide BATCH: every batch
    ends on a quad's last rank.  N = 8: a batch is exactly one quad of all ranks."""
    ex = set()
    if N == 1:
        ex |= {"rs_batch_splits_sum", "rs_empty_slice", "ag_skip", "ag_mixed_batch", "pub_peer_empty",
               "sgd:ag_mixed_batch"}
    if N in (2, 4, 8):
        ex |= {"rs_batch_splits_sum"}
    if N == 8:
        ex |= {"ag_mixed_batch", "sgd:ag_mixed_batch"}
    return ex


def required(N):
    return ALL_LABELS - exempt(N)


# ----------------------------------------------------------------------------------- cases
# sgd: None or the name of an option set of the GPU test; off: the bucket's offset in the data
# buffer; cap: add_channel's block count; pad: live elements behind the bucket (0: the bucket
# ends with the buffer); calls: calls per channel (>= 3: both stage parities twice over)
Case = namedtuple("Case", "name N n off cap sgd pad calls")
SGD_SETS = ("plain", "momentum", "nesterov_wd", "dampening_wd")
CALLS = 3


def _mk(N, tag, n, off, cap, sgd, pad=3):
    return Case("%s-n%d-off%d-b%d-%s" % (tag, n, off, cap, sgd or "nosgd"), N, n, off, cap, sgd, pad, CALLS)


def cases(N):
    """The shapes run at world size N.  Every case runs two-shot (plain, and with the publish
    pass and a prescale) and one-shot."""
    out = []
    small = sorted({1, 3, 4, 5, N - 1, 4 * N - 1, 4 * N, 4 * N + 1} - {0})
    offs = (0, 5, 6, 7, 4, 8, 9, 2)
    sets = (None,) + SGD_SETS
    for i, n in enumerate(small):
        out.append(_mk(N, "small", n, offs[i % len(offs)], 1, sets[i % len(sets)], pad=0 if i == 0 else 3))
    # tails of 1, 2, 3 elements in a rank's slice next to full quads, one rank without data
    for i, e in enumerate((1, 2, 3)):
        n = slice_len(4 * 7 * N + 1, N) * (N - 1) + 4 * 5 + e if N > 1 else 4 * 5 + e
        out.append(_mk(N, "tail", n, (4, 1, 8)[i], 1, SGD_SETS[(i + N) % 4]))
    q = 4 * THREADS
    # one block, the grid stride: three quads per thread and slice, the fourth for some (more
    # than one batch; N = 1 and 2 need nine and five quads per thread for a second batch)
    n = max(3, BATCH // N + 1) * q * N + 4 * 37 * N + 2
    out.append(_mk(N, "stride", n, 4, 1, "momentum"))
    out.append(_mk(N, "stride", n + 1, 3, 1, "nesterov_wd"))
    # two blocks, the second one partly filled; three blocks with two strides
    out.append(_mk(N, "blocks", q * N + 4 * 41 * N + 3, 8, 2, "dampening_wd"))
    out.append(_mk(N, "blocks", 3 * q * N + 4 * 50 * N + 5, 6, 2, "plain"))
    out.append(_mk(N, "blocks", 5 * q * N - 4 * 19 * N + 1, 0, 3, "momentum", pad=0))
    return out


def modes(case):
    """The (oneshot, publish, prescale) runs of a case; within one prescale all give the same bits."""
    ps = 1.0 / 3.0 if case.N in (1, 2, 4, 8) else 1.0 / case.N  # never a power of two
    return [(False, False, 1.0), (True, False, 1.0), (False, True, ps), (True, False, ps)]


@functools.lru_cache(maxsize=None)
def case_labels(case):
    """Every label the case's runs reach."""
    out = set()
    for oneshot, publish, _ in modes(case):
        nblk = blocks(case.n, case.N, oneshot, case.cap)
        got = paths(case.N, case.n, case.off, nblk, oneshot, publish)
        out |= got
        if case.sgd:
            out |= {"sgd:" + g for g in got if "sgd:" + g in SGD_LABELS}
    if case.calls >= 3:
        out.add("calls_both_parities")
    return out
