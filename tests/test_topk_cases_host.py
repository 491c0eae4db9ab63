"""CPU self-test of tests/topk_cases.py, the cases of tests/test_gpu_score_large_k.py: every case's preconditions hold (the
seeds are searched: nothing is left to luck on the GPU), check() accepts the reference -- also with every score moved by half
of what two float64 summation orders may differ by -- and rejects each defect the k > 16 routes could produce: a page cut
that repeats or skips a row, a tie in the wrong order, a shard base lost after the first page, a padding row, a second pool
that wrote over the first."""
import numpy as np
import pytest

from tests import topk_cases as TC

ALL = pytest.mark.parametrize("case", TC.CASES, ids=repr)


def _ref(case):
    ws, wi = TC.expected(case)
    return ws.copy(), wi.copy()


def _rejects(case, scores, ids):
    ws, wi = TC.expected(case)
    assert not (np.array_equal(scores, ws) and np.array_equal(ids, wi)), "the defect changed nothing"
    with pytest.raises(AssertionError):
        TC.check(case, scores, ids)


def test_the_list_is_the_one_the_issue_asks_for():
    got = {(c.Q, c.N, c.S, c.k) for c in TC.CASES}
    for shape in [(1, 100, 16, 90), (2, 33, 5, 33), (5, 3000, 32, 17), (33, 2000, 64, 64), (40, 700, 300, 40), (40, 700, 620, 40),
                  (3, 1100, 64, 1024), (3, 1100, 64, 1025), (3, 1100, 64, 1100), (2080, 300, 16, 20), (129, 9000, 64, 100),
                  (600, 6000, 64, 10), (1100, 6000, 64, 10)]:
        assert shape in got, shape
    assert len({c.name for c in TC.CASES}) == len(TC.CASES)
    by = TC.BY_NAME
    assert (by["tie_across_kth"].N, by["tie_across_kth"].S, by["tie_across_kth"].k, by["tie_across_kth"].copies) == (2000, 32, 20, 30)
    assert (by["zero_query_n3000"].N, by["zero_query_n3000"].k, by["zero_query_n5000"].N, by["zero_query_n5000"].k) == (3000, 40, 5000, 40)
    assert by["zero_query_n5000_base"].id_base == by["dup_overflow_base"].id_base == by["dev_index_id_base"].id_base == 1_000_000_007
    assert (by["dup_overflow"].N, by["dup_overflow"].S, by["dup_overflow"].k, by["dup_overflow"].copies, by["dup_overflow"].Q) == (6000, 64, 50, 4500, 8)
    assert by["strided_open_q600"].planted == (0, 299, 511, 599) and by["strided_open_q600"].copies == 4500
    assert by["slot_pool_exhausted"].copies == 600 and (by["slot_pool_exhausted"].collect, by["slot_pool_exhausted"].brute) == (1024, 76)
    # the counter deltas: every query is served exactly once, by the select kernel or by the brute force (pure paging: uncounted)
    for c in TC.CASES:
        if c.k > 16 and c.k <= 1024:
            assert c.collect + c.brute == c.Q, c
        elif c.k > 1024:
            assert (c.collect, c.brute) == (0, 0), c


@ALL
def test_preconditions(case):
    assert TC.preconditions(case)


def test_preconditions_of_a_larger_strided_case():
    """what the GPU test builds on a device with more than 300 CUs"""
    c = TC.strided_case(700)
    assert c.planted == (0, 349, 611, 699) and TC.preconditions(c)


def test_the_tie_group_reaches_the_places_it_is_meant_to():
    c = TC.BY_NAME["tie_across_kth"]
    _, _, group = TC.inputs(c)
    assert (group < 32).sum() >= 2 and (group >= (c.N // 32) * 32).sum() >= 2 and c.N % 32
    # the select route sweeps this index in 8 splits of 8 tiles (63 tiles; topk_select doubles nsplit up to 4 k candidates)
    assert len(set((group // 32) // 8)) == 8
    ws, wi = TC.expected(c)
    assert np.array_equal(wi[c.planted[0]], group[:20]) and (ws[c.planted[0]] == ws[c.planted[0], 0]).all()
    assert group[20:].size == 10                              # ten more copies tie with the 20th


def test_f64_rows_and_their_float32_rounding_have_different_references():
    a, b = TC.BY_NAME["f64_rows"], TC.BY_NAME["f64_rows_rounded"]
    ta, tb = TC.inputs(a)[1], TC.inputs(b)[1]
    assert ta.dtype == np.float64 and tb.dtype == np.float32 and np.array_equal(ta.astype(np.float32), tb)
    assert np.array_equal(TC.inputs(a)[0], TC.inputs(b)[0])
    # a scorer that read the float32 image of a float64 index is caught by the score bar
    assert np.abs(TC.expected(a)[0] - TC.expected(b)[0]).max() > 1e3 * TC.score_bar(a)


@ALL
def test_check_accepts_the_reference(case):
    ws, wi = _ref(case)
    assert TC.check(case, ws, wi) == 0.0


@ALL
def test_check_accepts_scores_moved_by_half_the_summation_tolerance(case):
    ws, wi = _ref(case)
    tol = TC.scales(case)[2]
    # up or down by the parity of the score's last bit: entries of an exact tie move together, as a device's would
    sign = np.where(ws.view(np.uint64) & np.uint64(1), 1.0, -1.0)
    moved = ws + sign * (tol / 2)
    assert not np.array_equal(moved, ws)
    assert 0 < TC.check(case, moved, wi) <= tol


@pytest.mark.parametrize("name,query", [("tie_across_kth", 4), ("zero_query_n3000", 2), ("zero_query_n5000_base", 2), ("dup_overflow", 3),
                                        ("slot_pool_exhausted", 1099)])
def test_check_rejects_a_reversed_tie(name, query):
    case = TC.BY_NAME[name]
    ws, wi = _ref(case)
    assert (ws[query] == ws[query, 0]).all()
    wi[query] = wi[query, ::-1]
    _rejects(case, ws, wi)
    ws, wi = _ref(case)                                       # one pair only, at the end of the first page
    if case.k > 16:
        wi[query, [15, 16]] = wi[query, [16, 15]]
        _rejects(case, ws, wi)


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.k > 16], ids=repr)
@pytest.mark.parametrize("at", ["16/17", "k-1/k"])
def test_check_rejects_two_neighbours_swapped(case, at):
    ws, wi = _ref(case)
    a = 15 if at == "16/17" else case.k - 2
    q = case.Q - 1
    ws[q, [a, a + 1]] = ws[q, [a + 1, a]]
    wi[q, [a, a + 1]] = wi[q, [a + 1, a]]
    _rejects(case, ws, wi)


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.k > 17], ids=repr)
def test_check_rejects_rank_17_repeating_rank_16(case):
    """a page cut that forgot the id rule"""
    ws, wi = _ref(case)
    ws[:, 16:] = ws[:, 15:-1]
    wi[:, 16:] = wi[:, 15:-1]
    _rejects(case, ws, wi)
    ws, wi = _ref(case)                                       # one query, one place
    ws[0, 16], wi[0, 16] = ws[0, 15], wi[0, 15]
    _rejects(case, ws, wi)


@pytest.mark.parametrize("case", [c for c in TC.CASES if 16 < c.k < c.N], ids=repr)
def test_check_rejects_rank_17_skipped(case):
    ws1, wi1 = TC.reference(case, case.k + 1)
    ws = np.concatenate([ws1[:, :16], ws1[:, 17:]], axis=1)
    wi = np.concatenate([wi1[:, :16], wi1[:, 17:]], axis=1)
    _rejects(case, ws, wi)


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.id_base], ids=repr)
def test_check_rejects_a_base_missing_after_the_first_page(case):
    ws, wi = _ref(case)
    wi[:, 16:] -= case.id_base
    _rejects(case, ws, wi)


@pytest.mark.parametrize("name", ["fewer_candidates_than_k", "k_is_n_tail_tile_of_one", "dev_index_id_base", "zero_query_n3000"])
def test_check_rejects_a_padding_row(name):
    case = TC.BY_NAME[name]
    for row in (case.N, (case.N + 31) // 32 * 32 - 1):       # the zero rows behind the last tile score 0
        ws, wi = _ref(case)
        wi[0, -1] = case.id_base + row
        _rejects(case, ws, wi)
        ws, wi = _ref(case)
        zq = case.zero[0] if case.zero else 0
        wi[zq, 5] = case.id_base + row
        _rejects(case, ws, wi)


def test_check_rejects_a_second_pool_that_repeats_the_first():
    case = TC.BY_NAME["second_pool"]
    assert case.Q == 2048 + 32
    ws, wi = _ref(case)
    ws[-32:], wi[-32:] = ws[:32], wi[:32]
    _rejects(case, ws, wi)
    ws, wi = _ref(case)                                       # or that was never written (NaN / -7 as the device test pre-fills)
    ws[-32:], wi[-32:] = np.nan, -7
    _rejects(case, ws, wi)


@ALL
def test_check_rejects_a_score_off_by_1e_9(case):
    for q, j, d in [(case.Q - 1, case.k - 1, -1e-9), (0, 0, 1e-9), (case.Q // 2, case.k // 2, 1e-9)]:
        ws, wi = _ref(case)
        ws[q, j] += d
        _rejects(case, ws, wi)


def test_check_rejects_wrong_types_and_shapes():
    case = TC.BY_NAME["k17"]
    ws, wi = _ref(case)
    with pytest.raises(AssertionError):
        TC.check(case, ws.astype(np.float32), wi)
    with pytest.raises(AssertionError):
        TC.check(case, ws[:, :16], wi[:, :16])
