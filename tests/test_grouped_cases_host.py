"""CPU self-test of tests/grouped_cases.py, the cases of tests/test_gpu_score_grouped.py: every case's preconditions hold,
check() accepts the reference and rejects each defect a grouped top-k could produce -- a group twice, a representative that is
not its group's best, a tie in the wrong order, a wrong count, a padding slot that holds something, an ineligible id, a score
off by more than the bar -- sharded.merge_grouped_lists on CPU tensors equals the reference over 2- and 3-way splits, and
sse_index.group_keys round-trips."""
import numpy as np
import pytest

from tests import grouped_cases as GC

ALL = pytest.mark.parametrize("case", GC.CASES, ids=repr)


def _ref(case):
    return tuple(a.copy() for a in GC.expected(case))


def _rejects(case, scores, ids, groups, counts):
    want = GC.expected(case)
    assert not all(np.array_equal(a, b) for a, b in zip((scores, ids, groups, counts), want)), "the defect changed nothing"
    with pytest.raises(AssertionError):
        GC.check(case, scores, ids, groups, counts)


def test_the_list_is_the_one_the_issue_asks_for():
    got = {(c.Q, c.N, c.S, c.k) for c in GC.CASES}
    for shape in [(5, 3000, 32, 10), (5, 3000, 32, 40), (9, 2000, 32, 20), (4, 500, 16, 10), (4, 5000, 16, 10), (2, 33, 5, 33), (2, 33, 5, 40),
                  (33, 2000, 64, 40), (40, 700, 300, 40), (40, 700, 620, 40), (3, 4000, 64, 1024), (8, 6000, 64, 50), (9, 1200, 40, 33)]:
        assert shape in got, shape
    assert len({c.name for c in GC.CASES}) == len(GC.CASES)
    by = GC.BY_NAME
    assert by["one_group"].counts == (1, 1, 1, 1) and by["three_groups"].counts == (3, 3, 3, 3)
    assert by["three_groups_n5000"].brute == by["three_groups_n5000"].Q == 4
    assert by["overflow_in_one_group"].brute == 1 and by["overflow_in_one_group"].base.copies == 4500
    assert by["tie_over_three_groups"].base.copies == by["tie_in_one_group"].base.copies == 30
    assert by["shard_base_dev"].id_base == by["shard_base_f64"].id_base == GC.BASE
    assert (by["shard_base_dev"].upload, by["shard_base_dev"].group_entry, by["shard_base_f64"].upload) == ("dev", "dev", "f64")
    assert by["own_group_k10"].same_as_topk and by["own_group_k40"].same_as_topk


@ALL
def test_preconditions(case):
    assert GC.preconditions(case)


def test_the_constructions_reach_what_they_are_meant_to():
    # keys over the whole int64 range
    g = GC.inputs(GC.BY_NAME["random_groups_of_8"])["groups"]
    assert (g < 0).any() and (g > 2 ** 40).any() and (g == GC.I64_MIN).any() and (g == GC.PAD).any()
    # best 100 in one group: the group leads every list, its second-best row is NOT in the list, rank 1 is unfiltered rank >= 100
    c = GC.BY_NAME["best_100_in_one_group"]
    I = GC.inputs(c)
    order = np.argsort(-I["s"], axis=1, kind="stable")
    ws, wi, wg, wc = GC.expected(c)
    assert (wg[:, 0] == 77).all() and np.array_equal(wi[:, 0], order[:, 0]) and (wc == c.k).all()
    for qi in range(c.Q):
        assert int(np.flatnonzero(order[qi] == wi[qi, 1])[0]) >= 100
    # ties: three representatives in id order, each the lowest copy of its group; one group: one entry
    c = GC.BY_NAME["tie_over_three_groups"]
    copies = GC.inputs(c)["copies"]
    ws, wi, wg, wc = GC.expected(c)
    assert wi[4, :3].tolist() == copies[:3].tolist() and ws[4, 0] == ws[4, 1] == ws[4, 2] > ws[4, 3]
    assert wg[4, :3].tolist() == [900, -900, 2 ** 41]
    c = GC.BY_NAME["tie_in_one_group"]
    ws, wi, wg, wc = GC.expected(c)
    assert wi[4, 0] == copies[0] and wg[4, 0] == 900 and ws[4, 1] < ws[4, 0] and not (wg[4, 1:] == 900).any()
    # overflow: the planted query returns the copies' group first, by the lowest copy
    c = GC.BY_NAME["overflow_in_one_group"]
    copies = GC.inputs(c)["copies"]
    ws, wi, wg, wc = GC.expected(c)
    assert wi[3, 0] == copies[0] and wg[3, 0] == 424242 and GC.brute_class(c) == ("no",) * 3 + ("yes",) + ("no",) * 4
    assert GC.brute_class(GC.BY_NAME["three_groups_n5000"]) == ("yes",) * 4
    # masks: the best group is gone, the next group is there but not by its best row
    c = GC.BY_NAME["masks_remove_and_demote"]
    I = GC.inputs(c)
    order = np.argsort(-I["s"], axis=1, kind="stable")
    ws, wi, wg, wc = GC.expected(c)
    e = GC.eligible(c)
    for qi in range(c.Q):
        best = I["groups"][order[qi, 0]]
        assert not (wg[qi] == best).any() and not e[qi, I["groups"] == best].any()
        nxt = next(r for r in order[qi] if I["groups"][r] != best)
        assert not e[qi, nxt] and I["groups"][nxt] in wg[qi].tolist()
        j = wg[qi].tolist().index(I["groups"][nxt])
        assert wi[qi, j] != nxt and I["s"][qi, wi[qi, j]] < I["s"][qi, nxt]
    # tail tile: the last row of the index is the best of query 0
    c = GC.BY_NAME["tail_tile_k40"]
    assert GC.expected(c)[1][0, 0] == 32 and (GC.expected(c)[1][:, 17:] == GC.PAD).all()
    # own groups: the reference is topk_cases' ranking
    c = GC.BY_NAME["own_group_k40"]
    from oracle import sse_oracle as O
    us, ui = O.topk(GC.inputs(c)["s"], c.k)
    assert np.array_equal(GC.expected(c)[1], ui) and np.array_equal(GC.expected(c)[0], us)


@ALL
def test_check_accepts_the_reference(case):
    assert GC.check(case, *_ref(case)) == 0.0


@ALL
def test_check_accepts_scores_moved_by_half_the_summation_tolerance(case):
    ws, wi, wg, wc = _ref(case)
    tol = GC.scales(case)[2]
    # equal scores move together (bit-equal rows have one score on any device)
    fin = np.where(np.isfinite(ws), ws, 0.0)
    moved = np.where(np.isfinite(ws), fin + np.where(np.floor(fin * 1e6) % 2 == 0, 1.0, -1.0) * (tol / 2), ws)
    assert not np.array_equal(moved, ws)
    assert GC.check(case, moved, wi, wg, wc) <= tol


@pytest.mark.parametrize("name,qi", [("random_groups_of_8", 0), ("best_100_in_one_group", 0), ("tie_over_three_groups", 4), ("k1024_groups_of_2", 0)])
def test_check_rejects_a_group_twice(name, qi):
    case = GC.BY_NAME[name]
    I = GC.inputs(case)
    ws, wi, wg, wc = _ref(case)
    rows = GC.ranking(case)[qi]
    mates = [r for r in rows if I["groups"][r] == wg[qi, 0] and r + case.id_base != wi[qi, 0]]
    assert mates, "the leading group has one eligible row"
    ws[qi, 1], wi[qi, 1], wg[qi, 1] = I["s"][qi, mates[0]], mates[0] + case.id_base, wg[qi, 0]   # the plain top-k's second column
    _rejects(case, ws, wi, wg, wc)


@pytest.mark.parametrize("name", ["random_groups_of_8", "masks_remove_and_demote", "tie_over_three_groups"])
def test_check_rejects_a_representative_that_is_not_the_best(name):
    case = GC.BY_NAME[name]
    I = GC.inputs(case)
    ws, wi, wg, wc = _ref(case)
    if name == "tie_over_three_groups":                       # an equal copy with a higher id: the same score, the wrong row
        copies = I["copies"]
        assert wi[4, 0] == copies[0] and I["groups"][copies[3]] == wg[4, 0]
        wi[4, 0] = copies[3]
    else:
        rows = GC.ranking(case)[0]
        for j in range(int(wc[0])):
            mates = [r for r in rows if I["groups"][r] == wg[0, j] and r + case.id_base != wi[0, j]]
            if mates:
                break
        assert mates
        ws[0, j], wi[0, j] = I["s"][0, mates[0]], mates[0] + case.id_base
    _rejects(case, ws, wi, wg, wc)


def test_check_rejects_the_ineligible_best_row_of_a_group():
    case = GC.BY_NAME["masks_remove_and_demote"]
    I = GC.inputs(case)
    order = np.argsort(-I["s"], axis=1, kind="stable")
    ws, wi, wg, wc = _ref(case)
    best = I["groups"][order[0, 0]]
    nxt = next(r for r in order[0] if I["groups"][r] != best)
    j = wg[0].tolist().index(I["groups"][nxt])
    ws[0, j], wi[0, j] = I["s"][0, nxt], nxt
    _rejects(case, ws, wi, wg, wc)
    ws, wi, wg, wc = _ref(case)                                # ... and the vanished group put back in front
    ws[0, 1:], wi[0, 1:], wg[0, 1:] = ws[0, :-1].copy(), wi[0, :-1].copy(), wg[0, :-1].copy()
    ws[0, 0], wi[0, 0], wg[0, 0] = I["s"][0, order[0, 0]], order[0, 0], best
    _rejects(case, ws, wi, wg, wc)


def test_check_rejects_two_tied_groups_swapped():
    case = GC.BY_NAME["tie_over_three_groups"]
    ws, wi, wg, wc = _ref(case)
    assert ws[4, 0] == ws[4, 1]
    wi[4, [0, 1]] = wi[4, [1, 0]]
    wg[4, [0, 1]] = wg[4, [1, 0]]
    _rejects(case, ws, wi, wg, wc)


@ALL
def test_check_rejects_a_wrong_count(case):
    for d in (1, -1):
        ws, wi, wg, wc = _ref(case)
        wc[case.Q - 1] += d
        _rejects(case, ws, wi, wg, wc)


@pytest.mark.parametrize("name", ["one_group", "three_groups", "tail_tile_k40"])
def test_check_rejects_a_padding_slot_that_holds_something(name):
    case = GC.BY_NAME[name]
    for what in ("id", "group", "score", "second_row_of_a_group"):
        ws, wi, wg, wc = _ref(case)
        c = int(wc[0])
        if what == "id":
            wi[0, -1] = case.id_base
        elif what == "group":
            wg[0, -1] = 3
        elif what == "score":
            ws[0, -1] = 0.0
        else:
            I = GC.inputs(case)
            r = next(r for r in GC.ranking(case)[0] if r + case.id_base not in wi[0, :c].tolist())
            ws[0, c], wi[0, c], wg[0, c] = I["s"][0, r], r + case.id_base, I["groups"][r]
        _rejects(case, ws, wi, wg, wc)


@ALL
def test_check_rejects_a_score_off_by_1e_9(case):
    ws, wi, wg, wc = _ref(case)
    qi = int(np.argmax(wc > 0))
    for j, d in [(0, 1e-9), (int(wc[qi]) - 1, -1e-9)]:
        ws, wi, wg, wc = _ref(case)
        ws[qi, j] += d
        _rejects(case, ws, wi, wg, wc)


def test_check_rejects_a_group_column_that_is_not_the_rows_key_and_wrong_types():
    case = GC.BY_NAME["random_groups_of_8"]
    ws, wi, wg, wc = _ref(case)
    wg[0, 0] += 1
    _rejects(case, ws, wi, wg, wc)
    ws, wi, wg, wc = _ref(case)
    with pytest.raises(AssertionError):
        GC.check(case, ws.astype(np.float32), wi, wg, wc)
    with pytest.raises(AssertionError):
        GC.check(case, ws, wi, wg.astype(np.int32), wc)
    with pytest.raises(AssertionError):
        GC.check(case, ws, wi, wg, wc.astype(np.int64))
    with pytest.raises(AssertionError):
        GC.check(case, ws[:, :5], wi[:, :5], wg[:, :5], wc)


# ---- the merge of the sharded call, on CPU tensors

def _local_lists(case, lo, hi, k):
    """what a rank holding rows [lo, hi) returns: the reference restricted to its rows, padded"""
    I = GC.inputs(case)
    ws = np.full((case.Q, k), -np.inf)
    wi = np.full((case.Q, k), GC.PAD, np.int64)
    wg = np.full((case.Q, k), GC.PAD, np.int64)
    for qi, rows in enumerate(GC.ranking(case)):
        rows = rows[(rows >= lo) & (rows < hi)]
        reps = GC.collapse(rows, I["groups"])[:k] if rows.size else rows
        c = reps.size
        ws[qi, :c], wi[qi, :c], wg[qi, :c] = I["s"][qi, reps], reps + case.id_base, I["groups"][reps]
    return ws, wi, wg


@pytest.mark.parametrize("name,cuts", [("random_groups_of_8", (1500,)), ("random_groups_of_8", (7, 2990)), ("best_100_in_one_group", (1000,)),
                                       ("three_groups", (250,)), ("three_groups", (100, 101)), ("one_group", (499,)),
                                       ("tie_over_three_groups", (1000,)), ("tie_in_one_group", (700, 1400)),
                                       ("masks_remove_and_demote", (1234,)), ("shard_base_f64", (400, 800)), ("tail_tile_k40", (33,))])
def test_merge_grouped_lists_equals_the_reference(name, cuts):
    import torch
    from sse_amd.sharded import merge_grouped_lists
    case = GC.BY_NAME[name]
    bounds = [0] + list(cuts) + [case.N]
    parts = [_local_lists(case, lo, hi, case.k) for lo, hi in zip(bounds[:-1], bounds[1:])]
    if name in ("best_100_in_one_group", "three_groups"):      # a group on both sides: the merge has something to drop
        both = [set(p[2][0][p[1][0] != GC.PAD].tolist()) for p in parts]
        assert both[0] & both[-1]
    if name == "tail_tile_k40":                                # the last shard is empty: an all-padding list
        assert (parts[-1][1] == GC.PAD).all()
    s, i, g = (torch.from_numpy(np.concatenate([p[j] for p in parts], axis=1)) for j in range(3))
    out = merge_grouped_lists(s, i, g, case.k)
    got = tuple(o.numpy() for o in out)
    assert got[3].dtype == np.int32
    for a, b in zip(got, GC.expected(case)):
        assert np.array_equal(a, b)
    GC.check(case, *got)


def test_merge_grouped_lists_of_nothing():
    import torch
    from sse_amd.sharded import merge_grouped_lists
    s = torch.full((3, 8), float("-inf"), dtype=torch.float64)
    i = torch.full((3, 8), GC.PAD, dtype=torch.int64)
    os_, oi, og, oc = merge_grouped_lists(s, i, i.clone(), 4)
    assert os_.shape == (3, 4) and bool((os_ == float("-inf")).all()) and bool((oi == GC.PAD).all()) and bool((og == GC.PAD).all())
    assert oc.tolist() == [0, 0, 0]
    # a real group that carries the padding key is kept, once
    s[0, 0], i[0, 0] = 0.5, 9
    s[0, 4], i[0, 4] = 0.25, 2
    g = torch.full((3, 8), GC.PAD, dtype=torch.int64)
    os_, oi, og, oc = merge_grouped_lists(s, i, g, 4)
    assert oc.tolist() == [1, 0, 0] and oi[0].tolist() == [9, GC.PAD, GC.PAD, GC.PAD] and os_[0, 0] == 0.5
    out = merge_grouped_lists(s[:0], i[:0], g[:0], 4)
    assert out[0].shape == (0, 4) and out[3].shape == (0,)


def test_group_keys_round_trip():
    from sse_amd.sse_index import group_keys
    labels = ["shoes", 7, "books", "shoes", 0, ("a", 1), 7, -3, 2 ** 63 - 1, np.int64(-2 ** 63), 2 ** 70, 1, "books"]
    keys, table = group_keys(labels)
    assert keys.dtype == np.int64 and keys.shape == (len(labels),)
    for lab, key in zip(labels, keys):
        assert table[lab] == int(key)
    assert len(set(table.values())) == len(table) == 10             # distinct labels, distinct keys
    for lab in (7, 0, -3, 2 ** 63 - 1, 1):
        assert table[lab] == lab                                    # an integer that fits is its own key
    assert table[np.int64(-2 ** 63)] == -2 ** 63
    assert table["shoes"] == 2 and table["books"] == 3 and table[("a", 1)] == 4 and table[2 ** 70] == 5   # the free keys from 0 up
    back = {k: lab for lab, k in table.items()}
    assert [back[int(k)] for k in keys] == labels
    keys, table = group_keys([])
    assert keys.shape == (0,) and table == {}
    keys, table = group_keys(np.arange(5) * 3)
    assert keys.tolist() == [0, 3, 6, 9, 12]
