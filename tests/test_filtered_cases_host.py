"""CPU self-test of tests/filtered_cases.py, the cases of tests/test_gpu_score_filtered.py: every case's preconditions hold,
check() accepts the reference and rejects each defect a filtered top-k could produce -- an ineligible id, a wrong count, a
padding slot that holds something, a tie in the wrong order, a missing row, a score off by more than the bar -- and
sse_index.tag_words round-trips."""
import numpy as np
import pytest

from tests import filtered_cases as FC

ALL = pytest.mark.parametrize("case", FC.CASES, ids=repr)


def _ref(case):
    ws, wi, wc = FC.expected(case)
    return ws.copy(), wi.copy(), wc.copy()


def _rejects(case, scores, ids, counts):
    ws, wi, wc = FC.expected(case)
    assert not (np.array_equal(scores, ws) and np.array_equal(ids, wi) and np.array_equal(counts, wc)), "the defect changed nothing"
    with pytest.raises(AssertionError):
        FC.check(case, scores, ids, counts)


def test_the_list_is_the_one_the_issue_asks_for():
    got = {(c.Q, c.N, c.S, c.k) for c in FC.CASES}
    for shape in [(5, 3000, 32, 10), (5, 3000, 32, 40), (9, 2000, 32, 20), (4, 500, 16, 10), (2, 33, 5, 33), (2, 33, 5, 40),
                  (33, 2000, 64, 40), (40, 700, 300, 40), (40, 700, 620, 40), (3, 5000, 64, 1024), (8, 6000, 64, 50), (6, 3000, 32, 10),
                  (9, 1200, 40, 33), (64, 4096, 32, 10)]:
        assert shape in got, shape
    assert len({c.name for c in FC.CASES}) == len(FC.CASES)
    by = FC.BY_NAME
    assert by["fewer_than_k"].counts == (3, 1, 0, 10)
    assert by["overflow"].brute == 1 and by["overflow"].base.copies == 4500 and sum(c.brute for c in FC.CASES) == 1
    assert by["tie_inside_k"].base.copies == 30 and by["tie_inside_k"].base.planted == (4,)
    assert by["shard_base_dev"].id_base == by["shard_base_f64"].id_base == FC.BASE
    assert (by["shard_base_dev"].upload, by["shard_base_dev"].tag_entry, by["shard_base_f64"].upload) == ("dev", "dev", "f64")
    assert FC.inputs(by["exclude_3_best"])["exclude"].shape == (6, 3) and FC.inputs(by["exclude_64_mixed"])["exclude"].shape == (6, 64)
    assert [v[1:] for v in by["sorted_tags"].variants] == [(1, "any", "pos"), (0, "any", 0), (1, "none", 0)]


@ALL
def test_preconditions(case):
    assert FC.preconditions(case)


def test_the_constructions_reach_what_they_are_meant_to():
    # best rows ineligible: the unfiltered top 100 of every query are out, so the answer starts at unfiltered rank 100
    c = FC.BY_NAME["best_rows_ineligible"]
    s = FC.inputs(c)["s"]
    order = np.argsort(-s, axis=1, kind="stable")
    assert np.array_equal(FC.expected(c)[1][:, 0], order[:, 100])
    # tie: fifteen eligible copies lead query 4 in id order, every second copy of the group is missing
    c = FC.BY_NAME["tie_inside_k"]
    group = FC.inputs(c)["group"]
    ws, wi, _ = FC.expected(c)
    assert np.array_equal(wi[4, :15], group[0::2]) and (ws[4, :15] == ws[4, 0]).all() and ws[4, 15] < ws[4, 0]
    # tail tile: the last row of the index is the best of query 0
    c = FC.BY_NAME["tail_tile_k40"]
    assert FC.expected(c)[1][0, 0] == 32 and (FC.expected(c)[1][:, 33:] == FC.PAD_ID).all()
    # exclusion lists: duplicates, -1, ids outside, ids the tags removed; the sixth best eligible row leads
    c = FC.BY_NAME["exclude_64_mixed"]
    I = FC.inputs(c)
    ex = I["exclude"]
    assert (ex == -1).any() and (ex >= c.N).any() and (ex < -1).any()
    for qi in range(c.Q):
        inside = ex[qi][(ex[qi] >= 0) & (ex[qi] < c.N)]
        assert len(set(inside.tolist())) < inside.size and (I["tags"][inside] != FC.bit(0)).any()
        el = np.flatnonzero(FC.eligible_by_tags(c)[qi])
        assert FC.expected(c)[1][qi, 0] == el[np.argsort(-I["s"][qi, el], kind="stable")[5]]
    # shard base: a local row number in the list excludes nothing
    c = FC.BY_NAME["shard_base_dev"]
    ex = FC.inputs(c)["exclude"]
    assert (ex[:, 2] < c.id_base).all() and (ex[:, :2] >= c.id_base).all()
    removed = FC.eligible_by_tags(c).sum(1) - FC.eligible(c).sum(1)
    assert ((removed >= 0) & (removed <= 2)).all() and removed.sum() > 0
    # sorted tags: the first query tile asks tag 0 alone, the block tags 0 and 1: 6 x 16 tiles of one query block can be skipped
    c = FC.BY_NAME["sorted_tags"]
    I = FC.inputs(c)
    assert (I["any"][:32] == FC.bit(0)).all() and int(np.bitwise_or.reduce(I["any"])) == 3
    sums = np.bitwise_or.reduce(I["tags"].reshape(-1, 32), axis=1)
    assert int(((sums & np.uint64(3)) == 0).sum()) == 96


@ALL
def test_check_accepts_the_reference(case):
    ws, wi, wc = _ref(case)
    assert FC.check(case, ws, wi, wc) == 0.0


@ALL
def test_check_accepts_scores_moved_by_half_the_summation_tolerance(case):
    ws, wi, wc = _ref(case)
    tol = FC.scales(case)[2]
    sign = np.where(ws.view(np.uint64) & np.uint64(1), 1.0, -1.0)
    moved = np.where(np.isfinite(ws), ws + sign * (tol / 2), ws)
    assert not np.array_equal(moved, ws) or not wc.any()
    assert FC.check(case, moved, wi, wc) <= tol


@pytest.mark.parametrize("case", [c for c in FC.CASES if FC.inputs(c)["tags"] is not None or FC.inputs(c)["exclude"] is not None], ids=repr)
def test_check_rejects_an_ineligible_id(case):
    e = FC.eligible(case)
    qi = int(np.argmax(FC.expected(case)[2] > 0))
    r = int(np.flatnonzero(~e[qi])[0])
    ws, wi, wc = _ref(case)
    wi[qi, 0] = case.id_base + r
    _rejects(case, ws, wi, wc)


@pytest.mark.parametrize("name", ["exclude_3_best", "best_rows_ineligible"])
def test_check_rejects_the_unfiltered_answer(name):
    case = FC.BY_NAME[name]
    s = FC.inputs(case)["s"]
    from oracle import sse_oracle as O
    us, ui = O.topk(s, case.k)
    _rejects(case, np.ascontiguousarray(us), ui.astype(np.int64) + case.id_base, np.full(case.Q, case.k, np.int32))


@ALL
def test_check_rejects_a_wrong_count(case):
    for d in (1, -1):
        ws, wi, wc = _ref(case)
        wc[case.Q - 1] += d
        _rejects(case, ws, wi, wc)


@pytest.mark.parametrize("name", ["fewer_than_k", "tail_tile_k33", "tail_tile_k40"])
def test_check_rejects_a_padding_slot_that_holds_something(name):
    case = FC.BY_NAME[name]
    e = FC.eligible(case)
    for what in ("id", "score", "zero_row"):
        ws, wi, wc = _ref(case)
        qi = int(np.argmin(wc))
        if what == "id":
            wi[qi, -1] = case.id_base + int(np.flatnonzero(e[qi])[0]) if e[qi].any() else case.id_base
        elif what == "score":
            ws[qi, -1] = 0.0
        else:
            ws[qi, wc[qi]], wi[qi, wc[qi]] = 0.0, case.id_base + case.N    # a zero row behind the last tile
        _rejects(case, ws, wi, wc)


@pytest.mark.parametrize("name,query", [("tie_inside_k", 4), ("overflow", 3)])
def test_check_rejects_two_tied_ids_swapped(name, query):
    case = FC.BY_NAME[name]
    ws, wi, wc = _ref(case)
    assert ws[query, 3] == ws[query, 4]
    wi[query, [3, 4]] = wi[query, [4, 3]]
    _rejects(case, ws, wi, wc)


@pytest.mark.parametrize("case", [c for c in FC.CASES if (FC.expected(c)[2] == c.k).any()], ids=repr)
def test_check_rejects_a_missing_row(case):
    ws1, wi1, wc1 = FC.reference(case, case.k + 1)
    qi = int(np.argmax(wc1 == case.k + 1))
    assert wc1[qi] == case.k + 1
    ws, wi, wc = _ref(case)
    j = case.k // 2
    ws[qi, j:], wi[qi, j:] = ws1[qi, j + 1:], wi1[qi, j + 1:]
    _rejects(case, ws, wi, wc)


@pytest.mark.parametrize("case", [c for c in FC.CASES if FC.expected(c)[2].any()], ids=repr)
def test_check_rejects_a_score_off_by_1e_9(case):
    ws, wi, wc = _ref(case)
    qi = int(np.argmax(wc > 0))
    for j, d in [(0, 1e-9), (int(wc[qi]) - 1, -1e-9)]:
        ws, wi, wc = _ref(case)
        ws[qi, j] += d
        _rejects(case, ws, wi, wc)


def test_check_rejects_wrong_types_and_shapes():
    case = FC.BY_NAME["one_of_eight"]
    ws, wi, wc = _ref(case)
    with pytest.raises(AssertionError):
        FC.check(case, ws.astype(np.float32), wi, wc)
    with pytest.raises(AssertionError):
        FC.check(case, ws, wi, wc.astype(np.int64))
    with pytest.raises(AssertionError):
        FC.check(case, ws[:, :5], wi[:, :5], wc)


def test_tag_words_round_trip_and_its_limit():
    from sse_amd.sse_index import tag_words
    groups = ["shoes", "books", "shoes", 7, "books", ("a", 1), 7]
    words, bits = tag_words(groups)
    assert words.dtype == np.uint64 and words.shape == (7,) and bits == {"shoes": 0, "books": 1, 7: 2, ("a", 1): 3}
    assert [int(w) for w in words] == [1, 2, 1, 4, 2, 8, 4]
    back = {b: g for g, b in bits.items()}
    assert [back[int(w).bit_length() - 1] for w in words] == groups
    words, bits = tag_words(list(range(64)))
    assert int(words[63]) == 1 << 63 and len(bits) == 64
    with pytest.raises(ValueError):
        tag_words(list(range(65)))
    words, bits = tag_words([])
    assert words.shape == (0,) and bits == {}
