"""The loopback all-reduce cases reach every path of the kernel's index plan at every world size.

tests/xgmi_cases.py replays which thread of xgmi_allreduce_body takes which item by which path;
here, for every N in 1..8 on its own, the union over the cases run on the GPU
(tests/test_xgmi_loopback_gpu.py) must hold every label that can occur at that N.  Removing a
case that alone carries a label for some N fails this file.  The model's slice / block
arithmetic and a few whole label sets are held against values worked out by hand."""
import pytest

import xgmi_cases as X

WORLDS = list(range(1, X.MAX_RANKS + 1))


def missing(N, cases):
    got = set()
    for c in cases:
        got |= X.case_labels(c)
    return X.required(N) - got


def test_slice_blocks_stage_by_hand():
    # n / N rounded up, then up to a whole quad
    assert X.slice_len(5, 3) == 4 and X.slice_len(10, 2) == 8 and X.slice_len(1, 8) == 4
    assert X.slice_len(33, 8) == 8 and X.slice_len(18816, 3) == 6272 and X.slice_len(501770, 2) == 250888
    assert X.slice_len(7, 1) == 8 and X.slice_len(4096, 8) == 512
    # one block per 256 quads of the slice (one-shot: of the bucket), 1..256, then the cap
    assert X.blocks(1, 8, False) == 1 and X.blocks(4 * 256, 1, False) == 1 and X.blocks(4 * 256 + 1, 1, False) == 2
    assert X.blocks(501770, 2, False) == 246 and X.blocks(18816, 2, True) == 19 and X.blocks(18816, 2, False) == 10
    assert X.blocks(10 ** 7, 2, False) == 256 and X.blocks(501770, 2, False, cap=3) == 3
    assert X.blocks(5, 3, False, cap=3) == 1
    assert X.stage_floats(5, 3, True) == 8 and X.stage_floats(5, 3, False) == 4 and X.stage_floats(8, 1, True) == 8


def test_paths_by_hand():
    # n = 5 over 3 ranks: slices of 4 - rank 0 a full quad, rank 1 one element, rank 2 nothing
    assert X.paths(3, 5, 0, 1, False, True) == {
        "pub_quad", "pub_elem", "pub_peer_empty", "rs_full_quad", "rs_short_slice", "rs_tail_1",
        "rs_tail_only_thread", "rs_empty_slice", "ag_vector", "ag_scalar_finish", "ag_skip"}
    # 513 full quads + 2 elements, one block of 256 threads: thread 0 sums quads (0, 256) and 512
    assert X.paths(2, 2054, 1, 1, True, False) == {
        "os_first_quad", "os_second_stride_full", "os_padded_tail", "os_paired", "os_odd_remainder",
        "os_off_unaligned"}
    # two quads per thread and slice at N = 3: one batch of 6 items, two quads x three ranks
    assert X.paths(3, 3 * 4 * 256 * 2, 0, 1, False, False) == {"rs_full_quad", "rs_grid_stride", "ag_vector",
                                                             "ag_mixed_batch"}
    # three: 9 items, the first batch ends after rank 1 of the third quad
    assert X.paths(3, 3 * 4 * 256 * 3, 0, 1, False, False) == {
        "rs_full_quad", "rs_grid_stride", "rs_multi_batch", "rs_batch_splits_sum", "ag_vector", "ag_mixed_batch",
        "ag_load_pm_later"}
    # N = 8: a batch is one quad of every rank, whatever the length
    assert "ag_mixed_batch" not in X.paths(8, 8 * 4 * 256 * 3, 0, 1, False, False)
    # an unaligned bucket never takes a vector store
    assert X.paths(2, 8, 6, 1, False, False) == {"rs_full_quad", "ag_off_2"}
    # 300 quads: the second block holds threads with and without a first quad
    assert "os_first_ok_mixed" in X.paths(1, 1200, 0, 2, True, False)
    assert "os_first_ok_mixed" not in X.paths(1, 4 * 256, 0, 1, True, False)


def test_exemptions_are_exactly_the_unreachable_labels():
    assert X.exempt(3) == X.exempt(5) == X.exempt(6) == X.exempt(7) == set()
    assert X.exempt(2) == X.exempt(4) == {"rs_batch_splits_sum"}
    assert X.exempt(8) == {"rs_batch_splits_sum", "ag_mixed_batch", "sgd:ag_mixed_batch"}
    assert X.exempt(1) == {"rs_batch_splits_sum", "rs_empty_slice", "ag_skip", "ag_mixed_batch", "pub_peer_empty",
                           "sgd:ag_mixed_batch"}
    for N in WORLDS:
        assert X.exempt(N) <= X.ALL_LABELS


@pytest.mark.parametrize("N", WORLDS)
def test_cases_reach_every_label(N):
    cases = X.cases(N)
    assert len({c.name for c in cases}) == len(cases)
    assert not missing(N, cases), sorted(missing(N, cases))
    # no case claims a label this N cannot reach (the exemption would be wrong)
    for c in cases:
        assert not X.case_labels(c) & X.exempt(N), (c.name, sorted(X.case_labels(c) & X.exempt(N)))
    # dropping a case that alone carries a label is noticed
    for c in cases:
        rest = [d for d in cases if d is not c]
        alone = X.case_labels(c) & X.required(N)
        for d in rest:
            alone -= X.case_labels(d)
        assert missing(N, rest) == alone, c.name


@pytest.mark.parametrize("N", WORLDS)
def test_case_shapes(N):
    """Small shapes, the lengths the plan's edges sit at, and a grid every block of which is
    resident at once."""
    cases = X.cases(N)
    ns = {c.n for c in cases}
    assert {1, 3, 4, 5, 4 * N - 1, 4 * N, 4 * N + 1} <= ns and (N == 1 or N - 1 in ns)
    assert {c.off % 4 for c in cases} == {0, 1, 2, 3}
    assert {c.cap for c in cases} == {1, 2, 3}
    assert {c.sgd for c in cases} == {None, *X.SGD_SETS}
    assert any(c.pad == 0 and c.off == 0 for c in cases)  # a bucket that is the whole buffer
    for c in cases:
        assert 1 <= c.n <= 3 * N * 4 * 256 * 3 + 4096 and c.calls >= 3
        for oneshot, _, _ in X.modes(c):
            assert N * X.blocks(c.n, N, oneshot, c.cap) <= X.GROUP_MAX_BLOCKS
