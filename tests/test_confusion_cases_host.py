"""CPU self-test of tests/confusion_cases.py: every case's preconditions hold, the reference passes its own check, and check()
rejects the defects a wrong sse_score_confusions would produce."""
import numpy as np
import pytest

from tests import confusion_cases as CC


def _exp(case):
    return tuple(np.array(a) for a in CC.expected(case))


@pytest.mark.parametrize("case", CC.CASES, ids=repr)
def test_preconditions_and_reference_passes(case):
    assert CC.preconditions(case)
    assert CC.check(case, *_exp(case)) == 0.0


def test_case_list_covers_what_the_stages_can_get_wrong():
    by = CC.BY_NAME
    assert {c.k for c in CC.CASES} >= {1, 17, 1024} and any(c.k > c.N for c in CC.CASES)
    assert {CC.inputs(c)["pos"].shape[1] for c in CC.CASES} >= {1, 3, 64}
    assert any(c.id_base and c.N % 32 == 20 for c in CC.CASES) and any(c.upload == "f64" and c.S == 50 for c in CC.CASES)
    assert any(c.margin == CC.INF for c in CC.CASES) and any(c.margin < 0 for c in CC.CASES)
    sh = by["shard_base_dev"]
    assert not CC.positive_rows(sh)[0].size and (CC.inputs(sh)["pos"][0] == -1).all()        # all padding
    assert CC.positive_rows(sh)[1][0] >= (sh.N // 32) * 32                                   # tail tile
    assert CC.positive_rows(sh)[2].size == 1 and (CC.inputs(sh)["pos"][2] >= 0).sum() == 2   # an id of another shard
    co = by["copies_on_floor"]
    p = co.base.planted[0]
    ws, wi, wc, wm, wb = CC.expected(co)
    g = CC.inputs(co)["group"]
    assert wc[p] == 28 and (ws[p, :28] == wm[p]).all() and wb[p] == g[3] + co.id_base
    assert by["overflow_floor_below"].brute == 1 and by["overflow_positive_above"].brute == 0
    assert by["overflow_positive_above"].floor == by["overflow_positive_above"].Q


def test_the_call_is_declared_and_bound():
    import os
    import sse_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sse_hip.h")).read()
    for name in ("sse_score_confusions", "sse_score_confusions_dev"):
        assert "int %s(sse_handle *h" % name in header and name in sse_amd.SYMBOLS
    assert "data.py:124-129" in header


def _rejected(case, res):
    with pytest.raises(AssertionError):
        CC.check(case, *res)


def test_check_rejects_a_positive_returned():
    case = CC.BY_NAME["three_above_margin0"]
    sc, ids, cnt, pm, pb = _exp(case)
    ids[1, 2] = pb[1]
    _rejected(case, (sc, ids, cnt, pm, pb))


def test_check_rejects_a_row_below_the_floor():
    case = CC.BY_NAME["three_above_margin0"]
    sc, ids, cnt, pm, pb = _exp(case)
    us, ui = CC.reference(case, cut=False)[:2]
    sc[0, 3], ids[0, 3], cnt[0] = us[0, 3], ui[0, 3], 4        # the best row under the positive
    assert us[0, 3] < pm[0]
    _rejected(case, (sc, ids, cnt, pm, pb))


def test_check_rejects_a_row_at_the_floor_dropped():
    case = CC.BY_NAME["copies_on_floor"]
    p = case.base.planted[0]
    sc, ids, cnt, pm, pb = _exp(case)
    assert sc[p, 27] == pm[p]                                  # the last copy sits on the floor exactly
    sc[p, 27], ids[p, 27], cnt[p] = -np.inf, CC.PAD_ID, 27
    _rejected(case, (sc, ids, cnt, pm, pb))


def test_check_rejects_a_wrong_tie_order():
    case = CC.BY_NAME["copies_on_floor"]
    p = case.base.planted[0]
    sc, ids, cnt, pm, pb = _exp(case)
    assert sc[p, 4] == sc[p, 5]
    ids[p, 4], ids[p, 5] = ids[p, 5], ids[p, 4]
    _rejected(case, (sc, ids, cnt, pm, pb))


def test_check_rejects_the_wrong_one_of_two_tied_positives():
    case = CC.BY_NAME["copies_on_floor"]
    sc, ids, cnt, pm, pb = _exp(case)
    pos = CC.inputs(case)["pos"]
    assert pb[0] == pos[0].min() and pos[0, 0] != pb[0]
    pb[0] = pos[0, 0]                                          # the first listed, not the lower id
    _rejected(case, (sc, ids, cnt, pm, pb))


def test_check_rejects_bad_padding():
    case = CC.BY_NAME["three_above_margin0"]
    for col, val in ((0, 0.0), (1, -1)):
        res = list(_exp(case))
        res[col][2, 5] = val
        _rejected(case, tuple(res))


def test_check_rejects_a_moved_best_positive_score():
    case = CC.BY_NAME["margin_tenth"]
    sc, ids, cnt, pm, pb = _exp(case)
    pm[0] += 1e-6
    _rejected(case, (sc, ids, cnt, pm, pb))


@pytest.mark.parametrize("case", CC.CASES, ids=repr)
def test_reference_arrays_is_the_case_reference(case):
    I = CC.inputs(case)
    for a, w in zip(CC.reference_arrays(I["s"], I["pos"], case.margin, case.k, case.id_base), CC.expected(case)):
        assert np.array_equal(a, w)
    if case.id_base == 0:
        same = np.arange(case.N)
        if I["group"].size:
            same[I["group"]] = I["group"][0]
        assert CC.rows_decidable(I["s"], I["pos"], case.margin, case.k, CC.score_bar(case), same).all()
