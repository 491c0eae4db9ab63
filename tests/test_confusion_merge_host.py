"""sharded.merge_confusion_lists on the CPU against the unsharded float64 reference of tests/confusion_cases.py: every shard's
list is what Handle.score_confusions returns for its rows with margin = +inf (its best k non-positives, its own best positive),
formed here in numpy from the case's reference scores.  Two and three uneven shards, id_base != 0, the best positive on one
shard only, no positive on any shard, a tie across a shard boundary."""
import numpy as np
import pytest
import torch

from oracle import sse_oracle as O
from tests import confusion_cases as CC

PAD = CC.PAD_ID


def _local(case, lo, hi, k):
    """what the shard holding rows [lo, hi) returns with margin = +inf: (scores [Q,k], ids [Q,k], m [Q], b [Q])"""
    s = CC.inputs(case)["s"]
    notpos = CC.confusions(case, cut=False)
    sc = np.full((case.Q, k), -np.inf)
    ids = np.full((case.Q, k), PAD, np.int64)
    m = np.full(case.Q, -np.inf)
    b = np.full(case.Q, PAD, np.int64)
    for qi in range(case.Q):
        cols = lo + np.flatnonzero(notpos[qi, lo:hi])
        c = min(k, cols.size)
        if c:
            ss, ii = O.topk(s[qi:qi + 1, cols], c)
            sc[qi, :c], ids[qi, :c] = ss[0], cols[ii[0]] + case.id_base
        rows = CC.positive_rows(case)[qi]
        rows = rows[(rows >= lo) & (rows < hi)]
        if rows.size:
            j = np.lexsort((rows, -s[qi, rows]))[0]
            m[qi], b[qi] = s[qi, rows[j]], rows[j] + case.id_base
    return sc, ids, m, b


def _merged(case, bounds):
    from sse_amd.sharded import merge_confusion_lists
    parts = [_local(case, lo, hi, case.k) for lo, hi in bounds]
    sc = torch.from_numpy(np.concatenate([p[0] for p in parts], axis=1))
    ids = torch.from_numpy(np.concatenate([p[1] for p in parts], axis=1))
    m = torch.from_numpy(np.stack([p[2] for p in parts]))
    b = torch.from_numpy(np.stack([p[3] for p in parts]))
    out = merge_confusion_lists(sc, ids, m, b, case.margin, case.k)
    assert out[2].dtype == torch.int32
    return tuple(t.numpy() for t in out), parts


def _same(case, got):
    for a, w in zip(got, CC.expected(case)):
        assert np.array_equal(a, w), case
    assert CC.check(case, *got) == 0.0


@pytest.mark.parametrize("name", ["three_above_margin0", "margin_inf_n64", "negative_margin", "margin_tenth", "shard_base_dev",
                                  "k1024_over_n", "copies_on_floor", "best_row_margin0"])
@pytest.mark.parametrize("cuts", [(0.37,), (0.2, 0.71)], ids=["two_uneven", "three_uneven"])
def test_merge_equals_the_unsharded_reference(name, cuts):
    case = CC.BY_NAME[name]
    edges = [0] + [int(c * case.N) for c in cuts] + [case.N]
    bounds = list(zip(edges[:-1], edges[1:]))
    assert len({hi - lo for lo, hi in bounds}) == len(bounds)          # uneven
    got, parts = _merged(case, bounds)
    _same(case, got)
    if name == "shard_base_dev":
        assert case.id_base != 0
        assert (got[4][0] == PAD) and all(p[3][0] == PAD for p in parts)       # query 0: no positive on any shard
        assert sum(int(p[3][1] != PAD) for p in parts) == 1                    # query 1: the best positive on one shard only
        assert got[2][0] == case.k                                             # no positive: no cut


def test_a_tie_across_a_shard_boundary():
    case = CC.BY_NAME["copies_on_floor"]
    g = CC.inputs(case)["group"]
    p = case.base.planted[0]
    cut = int(g[12]) + 1                                                       # copies on both sides; the two tied positives (g[3], g[7]) left
    got, parts = _merged(case, [(0, cut), (cut, case.N)])
    _same(case, got)
    assert (parts[0][0][p] == got[3][p]).sum() > 0 and (parts[1][0][p] == got[3][p]).sum() > 0
    cut = int(g[5])                                                            # the tied positives on different shards: the lower id wins
    got, parts = _merged(case, [(0, cut), (cut, case.N)])
    _same(case, got)
    assert parts[0][3][p] == g[3] and parts[1][3][p] == g[7] and parts[0][2][p] == parts[1][2][p] and got[4][p] == g[3]


def test_no_shards_and_no_queries():
    from sse_amd.sharded import merge_confusion_lists
    e = torch.empty
    sc, ids, cnt, m, b = merge_confusion_lists(e((3, 0), dtype=torch.float64), e((3, 0), dtype=torch.int64), e((0, 3), dtype=torch.float64),
                                               e((0, 3), dtype=torch.int64), 0.1, 5)
    assert sc.shape == (3, 5) and bool((sc == float("-inf")).all()) and bool((ids == PAD).all()) and not cnt.any()
    assert bool((m == float("-inf")).all()) and bool((b == PAD).all())
    out = merge_confusion_lists(e((0, 8), dtype=torch.float64), e((0, 8), dtype=torch.int64), e((2, 0), dtype=torch.float64),
                                e((2, 0), dtype=torch.int64), 0.0, 4)
    assert out[0].shape == (0, 4) and out[2].shape == (0,)
