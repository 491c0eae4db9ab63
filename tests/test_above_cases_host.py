"""CPU side of sse_score_above's tests: the constructions of tests/above_cases.py are exact in any summation order (so the GPU
tests may compare score BITS with numpy's), the reference comparison rejects every defect it is there to catch, and the
per-pair merge ShardedIndex.score_above uses gives the reference's result on CPU tensors."""
from fractions import Fraction

import numpy as np
import pytest

from tests import above_cases as AC
from tests import rank_cases as RC


def _two_orders(q, t):
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    fwd = np.zeros((q.shape[0], t.shape[0]))
    for d in range(q.shape[1]):
        fwd += q64[:, d:d + 1] * t64[:, d][None, :]
    rev = np.zeros_like(fwd)
    for d in range(q.shape[1] - 1, -1, -1):
        rev += q64[:, d:d + 1] * t64[:, d][None, :]
    return fwd, rev


def _fraction_scores(q, t, rows):
    return [sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(q, t[r])) for r in rows]


def test_ladder_is_exact_and_dials_every_count():
    q, t, pi = AC.ladder_case()
    N = t.shape[0]
    fwd, rev = _two_orders(q, t)
    assert np.array_equal(fwd, rev) and np.array_equal(fwd, q.astype(np.float64) @ t.astype(np.float64).T)
    rows = np.random.RandomState(0).choice(N, size=50, replace=False)
    assert [Fraction(float(fwd[0, r])) for r in rows] == _fraction_scores(q[0], t, rows)
    assert np.array_equal(fwd[0], (pi + 1) * 2.0 ** -15)                  # strictly increasing in pi(r), 2^-15 apart
    assert 2.0 ** -15 > 2 * (2 * (64 + 2) * 5.97e-8)                      # wider than the whole fp32 band [s - e, s + e], max|t| < 1
    for c in AC.ladder_counts():
        assert int((fwd[0] >= AC.ladder_threshold(c)).sum()) == c
    assert AC.LADDER_N * 16 > 160 * 1024                                  # the whole ladder cannot be one LDS sort


def test_quarter_construction_is_exact():
    q, t = RC.quarter_set(61, 3, 2000, 64)
    fwd, rev = _two_orders(q, t)
    assert np.array_equal(fwd, rev) and np.array_equal(fwd, q.astype(np.float64) @ t.astype(np.float64).T)
    rows = np.random.RandomState(1).choice(2000, size=40, replace=False)
    assert [Fraction(float(fwd[0, r])) for r in rows] == _fraction_scores(q[0], t, rows)
    assert len(np.unique(fwd[0])) < 400                                   # a tie group at every distinct value


def _reference():
    q, t = RC.quarter_set(5, 4, 60, 16)
    t[50] = t[7]
    scores = q.astype(np.float64) @ t.astype(np.float64).T
    pair_q = np.array([0, 1, 2, 3, 0], np.int32)
    thr = np.array([scores[0, 7], scores[1, 7], scores[2, 7], np.inf, -np.inf])
    return scores, pair_q, thr, AC.expected_above(scores, pair_q, thr, id_base=100)


def test_reference_by_hand():
    scores, pair_q, thr, (off, ids, sc) = _reference()
    assert off[0] == 0 and off[-1] == len(ids) == len(sc)
    assert off[4] - off[3] == 0 and off[5] - off[4] == 60
    for p in range(5):
        seg_i, seg_s = ids[off[p]:off[p + 1]] - 100, sc[off[p]:off[p + 1]]
        assert set(seg_i.tolist()) == set(np.flatnonzero(scores[pair_q[p]] >= thr[p]).tolist())
        assert np.array_equal(seg_s, scores[pair_q[p], seg_i])
        assert all(seg_s[i] > seg_s[i + 1] or (seg_s[i] == seg_s[i + 1] and seg_i[i] < seg_i[i + 1]) for i in range(len(seg_i) - 1))
    seg0 = (ids[off[0]:off[1]] - 100).tolist()
    assert seg0[-2:] == [7, 50] or (7 in seg0 and 50 in seg0 and seg0.index(7) < seg0.index(50))
    nan = AC.expected_above(scores, [0], [np.nan])
    assert nan[0].tolist() == [0, 0] and len(nan[1]) == 0


def _drop_tie(off, ids, sc):
    """a tie at the threshold dropped: the last entry of segment 0 (row 50, tied with row 7 AT the threshold) is missing"""
    k = off[1] - 1
    o = off.copy()
    o[1:] -= 1
    return o, np.delete(ids, k), np.delete(sc, k)


def _ties_descending(off, ids, sc):
    i = ids.copy()
    k = off[1]
    assert sc[k - 1] == sc[k - 2]
    i[k - 2], i[k - 1] = ids[k - 1], ids[k - 2]
    return off, i, sc


def _offsets_off_by_one(off, ids, sc):
    o = off.copy()
    o[2] += 1
    return o, ids, sc


def _segment_unsorted(off, ids, sc):
    i, s = ids.copy(), sc.copy()
    a, b = off[4], off[4] + 30
    assert sc[a] != sc[b]
    i[a], i[b], s[a], s[b] = ids[b], ids[a], sc[b], sc[a]
    return off, i, s


def _local_ids(off, ids, sc):
    return off, ids - 100, sc


@pytest.mark.parametrize("defect", [_drop_tie, _ties_descending, _offsets_off_by_one, _segment_unsorted, _local_ids])
def test_comparison_rejects_each_defect(defect):
    _, _, _, want = _reference()
    AC.assert_above_equal(want, want)
    with pytest.raises(AssertionError):
        AC.assert_above_equal(defect(*want), want)


def test_shard_merge_on_cpu_tensors_gives_the_reference():
    import importlib
    import torch
    merge_above_runs = importlib.import_module("sse_amd.sharded").merge_above_runs
    q, t = RC.quarter_set(51, 5, 600, 64)
    t[500] = t[10]                                                        # a tie across the cuts
    scores = q.astype(np.float64) @ t.astype(np.float64).T
    pair_q = np.array([0, 1, 2, 3, 4, 0, 1], np.int32)
    thr = np.array([scores[0, 10], scores[1, 10], scores[2, 10], np.inf, -np.inf, np.quantile(scores[0], 0.9), np.nan])
    want = AC.expected_above(scores, pair_q, thr)
    L = len(thr)
    parts = [AC.expected_above(scores[:, a:b], pair_q, thr, id_base=a) for a, b in ((0, 200), (200, 200), (200, 600))]   # one empty shard
    pair = torch.cat([torch.repeat_interleave(torch.arange(L), torch.from_numpy(np.diff(p[0]))) for p in parts])
    got = merge_above_runs(pair, torch.cat([torch.from_numpy(p[2]) for p in parts]), torch.cat([torch.from_numpy(p[1]) for p in parts]), L)
    AC.assert_above_equal(tuple(x.numpy() for x in got), want)
    empty = merge_above_runs(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.int64), 3)
    assert empty[0].tolist() == [0, 0, 0, 0] and empty[1].numel() == 0


def test_near_duplicate_construction():
    t = AC.near_duplicate_rows()
    scores = t.astype(np.float64) @ t.astype(np.float64).T
    pairs = AC.expected_near_duplicates(scores, 0.999)
    assert len(pairs) == 17 and all(i < j for i, j, _ in pairs) and pairs == sorted(pairs)
    assert sum(s > 0.99999 for _, _, s in pairs) == 12 and np.abs(scores - 0.999).min() > 1e-9
