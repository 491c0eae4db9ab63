"""CPU checks behind the rank feature: the metric arithmetic of Evaluator.rank_metrics on hand-made ranks (unweighted batch
mean, multi-label sources), and the proof that the constructions of tests/rank_cases.py -- exact ties, near ties below fp32
resolution, the tie across a shard cut -- have float64 scores that are EXACT in any summation order, which is what lets
tests/test_gpu_score_rank.py demand equal ranks from a device that sums in its own order."""
from fractions import Fraction

import numpy as np
import pytest

from tests import rank_cases as RC


def test_rank_metrics_on_hand_made_ranks():
    from sse_amd.sse_evaluator import rank_metrics_from_ranks
    # 5 sources, batches of 2 -> [2, 2, 1] sources; labels per source: 1, 2, 1, 3, 2
    ranks = [np.array([0]), np.array([4, 1]), np.array([9]), np.array([2, 0, 30]), np.array([10, 11])]
    m = rank_metrics_from_ranks(ranks, top_n=(1, 3, 10), batch=2)
    best = np.array([0, 1, 9, 0, 10])
    assert m["mrr"] == pytest.approx(np.mean(1.0 / (1 + best)), abs=0, rel=1e-15)
    assert m["mean_rank"] == pytest.approx(np.mean(1 + best), abs=0, rel=1e-15)
    assert m["median_rank"] == 2.0
    # tight accuracy: share of a source's labels inside the top n, batch means averaged UNWEIGHTED (the last batch of one
    # source counts as much as the full ones)
    top1 = np.mean([(1.0 + 0.0) / 2, (0.0 + 1.0 / 3) / 2, 0.0 / 1])
    top3 = np.mean([(1.0 + 0.5) / 2, (0.0 + 2.0 / 3) / 2, 0.0 / 1])
    top10 = np.mean([(1.0 + 1.0) / 2, (1.0 + 2.0 / 3) / 2, 0.0 / 1])
    assert m["tight_acc"] == [top1, top3, top10]
    # weighted by source count instead, top-1 would be (1 + 0 + 0 + 1/3 + 0) / 5
    assert m["tight_acc"][0] != pytest.approx((1 + 1.0 / 3) / 5)


def test_tight_accuracy_is_the_evaluators_own_arithmetic():
    """rank < n per label == label in ranked[:n]: the dict's tight_acc repeats topk_tight_accuracy + the unweighted mean of
    Evaluator.eval bit for bit on a full ranking."""
    from sse_amd.sse_evaluator import rank_metrics_from_ranks, topk_tight_accuracy
    rng = np.random.RandomState(0)
    N, n_src, batch = 23, 31, 7
    ranked = np.array([rng.permutation(N) for _ in range(n_src)])
    labels = [list(rng.choice(N, size=rng.randint(1, 4), replace=False)) for _ in range(n_src)]
    ranks = [np.array([int(np.flatnonzero(ranked[i] == lab)[0]) for lab in labels[i]]) for i in range(n_src)]
    m = rank_metrics_from_ranks(ranks, top_n=(1, 3, 10), batch=batch)
    for j, n in enumerate((1, 3, 10)):
        accs = [topk_tight_accuracy(n, labels[b0:b0 + batch], ranked[b0:b0 + batch, :10]) for b0 in range(0, n_src, batch)]
        assert m["tight_acc"][j] == np.mean(accs)


def test_eval_ranks_flag_defaults_to_off():
    from sse_amd import sse_train
    assert sse_train.FLAGS.parse([]).eval_ranks == 0
    assert sse_train.FLAGS.parse(["--eval_ranks", "1"]).eval_ranks == 1


def _two_orders(q, t):
    """float64 scores summed forwards and backwards over the dimension"""
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    fwd = np.zeros((q.shape[0], t.shape[0]))
    bwd = np.zeros_like(fwd)
    S = q.shape[1]
    for d in range(S):
        fwd += np.outer(q64[:, d], t64[:, d])
        bwd += np.outer(q64[:, S - 1 - d], t64[:, S - 1 - d])
    return fwd, bwd


def _fraction_dot(qrow, trow):
    return sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(qrow, trow)), Fraction(0))


def _assert_exact(q, t, sample):
    fwd, bwd = _two_orders(q, t)
    assert np.array_equal(fwd, bwd)
    assert np.array_equal(fwd, np.dot(q.astype(np.float64), t.astype(np.float64).T))
    for qi, ti in sample:
        assert Fraction(float(fwd[qi, ti])) == _fraction_dot(q[qi], t[ti])


def test_exact_tie_constructions_are_exact_in_float64():
    rng = np.random.RandomState(0)
    q, t, copies = RC.exact_ties_case()
    N = t.shape[0]
    _assert_exact(q, t, [(0, int(copies[0])), (0, 3), (1, N - 1)] + [(int(rng.randint(5)), int(rng.randint(N))) for _ in range(20)])
    assert np.array_equal(t[N - 1], t[3]) and len(copies) == 31 and (t[copies] == t[copies[0]]).all()
    sc = np.dot(q.astype(np.float64), t.astype(np.float64).T)
    assert (np.sort(np.flatnonzero(sc[0] == sc[0].max())) == copies).all()        # the copies are query 0's strict maxima
    q, t = RC.shard_case()
    _assert_exact(q, t, [(0, 10), (0, 4000), (16, 4098)] + [(int(rng.randint(17)), int(rng.randint(4099))) for _ in range(20)])
    assert np.array_equal(t[4000], t[10])


@pytest.mark.parametrize("n_cluster,N", [(200, 1000), (5000, 6000)])
def test_near_tie_constructions_are_exact_and_inside_one_fp32_band(n_cluster, N):
    q, t, where = RC.near_tie_case(n_cluster, N)
    rng = np.random.RandomState(1)
    _assert_exact(q, t, [(0, int(where[0])), (1, int(where[-1]))] + [(int(rng.randint(2)), int(rng.randint(N))) for _ in range(20)])
    sc = np.dot(q.astype(np.float64), t.T)
    assert np.array_equal(sc[0, where], 0.5 + np.arange(n_cluster) * 2.0 ** -30)  # strictly increasing in i, exactly
    assert (np.diff(sc[1, where]) > 0).all()
    # one fp32 band: the spread of the cluster plus the float32 rounding of its rows stays under the bound the sweep
    # certifies with, 2 (S + 2) 5.97e-8 |q| max|t| (max|t| >= the cluster rows' own norm)
    S = q.shape[1]
    t32 = t.astype(np.float32)
    norm_max = float(np.sqrt((t32.astype(np.float64) ** 2).sum(1).max()))
    for qi in range(2):
        e = 2.0 * (S + 2) * 5.97e-8 * norm_max * float(np.linalg.norm(q[qi]))
        x32 = t32[where, 0].astype(np.float64) * float(q[qi, 0])                   # what an fp32 sweep sees of the cluster
        s64 = sc[qi, where]
        assert max(x32.max() - s64.min(), s64.max() - x32.min()) < e
