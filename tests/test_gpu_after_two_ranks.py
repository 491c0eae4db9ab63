"""ShardedIndex.score_topk_after as REAL ranks: processes on the one GPU of a test box, a `gloo` group between them (host-staged
collectives), each holding its rows and tag words only and all of them the same GLOBAL cursors.  Two ranks over uneven shards
(4099 rows: 2050 + 2049, id_base 2050 on rank 1) with an exact tie across the boundary and the cursor on its rank-0 row, so that
the first row after it lives on rank 1; cursors that are rows of either shard, +inf, NaN; a second page chained from the first
on every rank.  Three ranks over a two-row index (rank 2 holds nothing, k exceeds the rows).  The result on EVERY rank must equal
the single-handle call on the whole index -- including the (-inf, INT64_MAX) padding the merge writes into every slot past the
real entries.  One launch of tests/after_two_rank_worker.py per rank (tests/rank_launch.py); a child
that fails ends the launch and the other children are killed; a child that died of a signal ends the pytest session."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import after_cases as AC
from tests import filtered_cases as FC
from tests import rank_cases as RC
from tests.after_two_rank_worker import next_cursors
from tests.util import make_pair, model_params
from tests.rank_launch import free_port, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "after_two_rank_worker.py")


def _single_handle(q, t, tags, any_, cs, ci, k):
    """pages 1 and 2 and the cursor-free page of the unsharded handle, each held to the float64 oracle (scores exact in any
    order: the quarter construction)"""
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    h = m.handle
    h.index_upload(t)
    h.index_set_tags(tags)
    s = O.scores_f64(q, t.astype(np.float64))
    o = np.argsort(-s, axis=1, kind="stable")
    fs, fi = np.take_along_axis(s, o, 1), o.astype(np.int64)
    ok = ((any_[:, None] == 0) | ((tags[o] & any_[:, None]) != 0))
    want = {}
    for page in (1, 2):
        got = h.score_topk_after(q, k, after=(cs, ci), any_of=any_)
        for a, b in zip(got, AC.after_on_host(fs, fi, k, (cs, ci), ok)):
            assert np.array_equal(a, b), page
        want[page] = got
        cs, ci = next_cursors(cs, ci, *got)
    want[0] = h.score_topk_after(q, k, any_of=any_)
    for a, b in zip(want[0], AC.after_on_host(fs, fi, k, None, ok)):
        assert np.array_equal(a, b)
    h.close()
    return want


def _check_ranks(out, want):
    for r in range(len(out)):
        for page in (0, 1, 2):
            assert np.array_equal(out[r]["ids%d" % page], want[page][1]), "rank %d page %d" % (r, page)
            assert np.array_equal(out[r]["scores%d" % page], want[page][0]), "rank %d page %d" % (r, page)
            assert np.array_equal(out[r]["counts%d" % page], want[page][2]) and out[r]["counts%d" % page].dtype == np.int32
        assert str(out[r]["bad_k"]).startswith("ValueError")
        assert int(out[r]["bruteforce"]) == 0


def test_after_on_two_ranks_equals_the_single_handle(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.shard_case()                                       # multiples of 1/4: exact in any order; row 4000 == row 10
    N, Q, k = t.shape[0], q.shape[0], 8
    bounds = shard_bounds(N, 2)
    assert bounds == [(0, 2050), (2050, 4099)]                   # uneven; rank 1's id_base is 2050
    cut = bounds[1][0]
    b = int(np.argmax((t.astype(np.float64) ** 2).sum(1)))       # the row of largest norm: it and its copies are the strict
    assert b > cut                                               # maxima of the query equal to it (Cauchy-Schwarz)
    t[cut - 1] = t[cut] = t[b]                                   # a tie across the boundary itself
    q[0] = t[b]
    rng = np.random.RandomState(7)
    tags = (FC.U1 << rng.randint(0, 4, size=N).astype(np.uint64)).astype(np.uint64)
    tags[[b, cut - 1, cut]] = FC.bit(0)
    any_ = np.zeros(Q, np.uint64)
    any_[3::2] = (FC.bit(0) | FC.bit(1))
    s = O.scores_f64(q, t.astype(np.float64))
    o = np.argsort(-s, axis=1, kind="stable")
    # cursors: a row of the ranking -- of whichever shard -- per query, depth 0 .. 40
    depth = rng.randint(0, 41, size=Q)
    ci = o[np.arange(Q), depth].astype(np.int64)
    cs = s[np.arange(Q), ci].copy()
    cs[0], ci[0] = s[0, b], cut - 1                              # the rank-0 row of the boundary tie: row `cut` of rank 1 is next
    cs[1], cs[2] = np.inf, np.nan
    assert (ci[3:] < cut).any() and (ci[3:] >= cut).any()        # cursor rows on both ranks
    want = _single_handle(q, t, tags, any_, cs, ci, k)
    assert want[1][1][0, :2].tolist() == [cut, b] and want[1][0][0, 1] == s[0, b] and want[1][0][0, 2] < s[0, b]
    assert np.array_equal(want[1][1][1], want[0][1][1]) and want[1][2][2] == 0 and want[2][2][2] == 0
    assert (want[2][2][[0, 1] + list(range(3, Q))] == k).all()
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, tags=tags, any=any_, cs=cs, ci=ci)
    job = dict(world=2, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(x) for x in bounds], k=k)
    _check_ranks(launch(WORKER, tmp, 2, job), want)


def test_after_with_an_empty_shard(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.quarter_set(52, 3, 2, 16)
    bounds = shard_bounds(2, 3)
    assert bounds == [(0, 1), (1, 2), (2, 2)]                    # rank 2 holds nothing
    tags = np.array([FC.bit(0), FC.bit(1)], np.uint64)
    any_ = np.zeros(3, np.uint64)
    s = O.scores_f64(q, t.astype(np.float64))
    best = np.argmax(s, axis=1)
    cs = np.array([np.inf, s[1, best[1]], np.nan])               # everything; what follows the best row; nothing
    ci = np.array([0, best[1], 0], np.int64)
    k = 4                                                        # more than the index has rows
    want = _single_handle(q, t, tags, any_, cs, ci, k)
    assert want[1][2].tolist() == [2, 1, 0] and want[2][2].tolist() == [0, 0, 0] and want[0][2].tolist() == [2, 2, 2]
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, tags=tags, any=any_, cs=cs, ci=ci)
    job = dict(world=3, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(x) for x in bounds], k=k)
    _check_ranks(launch(WORKER, tmp, 3, job), want)
