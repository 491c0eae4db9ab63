"""ShardedIndex.score_topk_filtered as REAL ranks: processes on the one GPU of a test box, a `gloo` group between them
(host-staged collectives), each holding its rows and tag words only.  Two ranks over uneven shards (4099 rows: 2050 + 2049) with
an exact tie across the boundary whose rows are both eligible, a query whose eligible rows all live on rank 1, one with fewer
than k eligible rows in total, one with none, and exclusion lists holding ids of both shards; three ranks over a two-row index
(rank 2 holds nothing, k exceeds the rows).  The result on EVERY rank must equal the single-handle call on the whole index --
including the (-inf, INT64_MAX) padding the merge writes into every slot past the real entries.  One launch of
tests/filtered_two_rank_worker.py per rank; a child that fails, or the cap, ends the launch and the other children are killed;
a child that died of a signal ends the pytest session -- nothing more starts on the GPU after a fault."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import filtered_cases as FC
from tests import rank_cases as RC
from tests.util import make_pair, model_params
from tests.rank_launch import free_port, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "filtered_two_rank_worker.py")


def _reference(q, t, tags, any_, none_, ex, k):
    """the float64 oracle of the whole index (scores exact in any order: the quarter construction)"""
    s = O.scores_f64(q, t.astype(np.float64))
    Q, N = s.shape
    e = ((any_[:, None] == 0) | ((tags[None, :] & any_[:, None]) != 0)) & ((tags[None, :] & none_[:, None]) == 0)
    ws, wi, wc = np.full((Q, k), -np.inf), np.full((Q, k), FC.PAD_ID, np.int64), np.zeros(Q, np.int32)
    for qi in range(Q):
        r = ex[qi][(ex[qi] >= 0) & (ex[qi] < N)]
        e[qi, r] = False
        cols = np.flatnonzero(e[qi])
        c = min(k, cols.size)
        if c:
            ss, ii = O.topk(s[qi:qi + 1, cols], c)
            ws[qi, :c], wi[qi, :c], wc[qi] = ss[0], cols[ii[0]], c
    return ws, wi, wc


def _single_handle(q, t, tags, any_, none_, ex, k):
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    m.handle.index_upload(t)
    m.handle.index_set_tags(tags)
    want = m.handle.score_topk_filtered(q, k, any_of=any_, none_of=none_, exclude=ex)
    m.handle.close()
    ref = _reference(q, t, tags, any_, none_, ex, k)
    for a, b in zip(want, ref):
        assert np.array_equal(a, b)
    return want


def _check_ranks(out, want):
    for r in range(len(out)):
        assert np.array_equal(out[r]["ids"], want[1]), "rank %d" % r
        assert np.array_equal(out[r]["scores"], want[0]), "rank %d" % r
        assert np.array_equal(out[r]["counts"], want[2]) and out[r]["counts"].dtype == np.int32, "rank %d" % r
        assert str(out[r]["bad_k"]).startswith("ValueError")
        assert int(out[r]["bruteforce"]) == 0


def test_filtered_topk_on_two_ranks_equals_the_single_handle(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.shard_case()                                       # multiples of 1/4: exact in any order; row 4000 == row 10
    N, Q, k = t.shape[0], q.shape[0], 8
    bounds = shard_bounds(N, 2)
    assert bounds == [(0, 2050), (2050, 4099)]                   # uneven
    cut = bounds[1][0]
    b = int(np.argmax((t.astype(np.float64) ** 2).sum(1)))       # the row of largest norm: it and its copies are the strict
    assert b not in (cut - 1, cut)                               # maxima of the query equal to it (Cauchy-Schwarz)
    t[cut - 1] = t[cut] = t[b]                                   # a tie across the boundary itself
    q[0] = t[b]
    rng = np.random.RandomState(7)
    tags = (FC.bit(0) | (FC.U1 << rng.randint(1, 4, size=N).astype(np.uint64))).astype(np.uint64)
    tags[rng.choice(np.arange(cut, N), 30, replace=False)] |= FC.bit(5)      # rank 1 only
    tags[[5, 700, 2049]] |= FC.bit(6)                                         # three rows of rank 0 ...
    tags[[2050, 4098]] |= FC.bit(6)                                           # ... two of rank 1: five in all, fewer than k
    any_ = (FC.U1 << rng.randint(0, 4, size=Q).astype(np.uint64)).astype(np.uint64)
    any_[0], any_[1], any_[2], any_[3], any_[4] = FC.bit(0), FC.bit(5), FC.bit(6), FC.bit(7), np.uint64(0)
    none_ = np.zeros(Q, np.uint64)
    none_[5:] = FC.bit(3)
    s = O.scores_f64(q, t.astype(np.float64))
    ex = np.full((Q, 4), -1, np.int64)
    ex[:, 0] = np.argmax(s[:, :cut], axis=1)                     # the best row of either shard
    ex[:, 1] = cut + np.argmax(s[:, cut:], axis=1)
    ex[:, 2] = N + 3
    ex[0, :2] = [3, N - 1]                                       # (query 0 keeps its three tied maxima)
    want = _single_handle(q, t, tags, any_, none_, ex, k)
    assert want[1][0, :3].tolist() == sorted([b, cut - 1, cut]) and want[0][0, 0] == want[0][0, 2]
    assert (want[1][1, :want[2][1]] >= cut).all() and want[2][1] == k        # every eligible row on rank 1
    assert want[2][2] == 5 and (want[1][2, 5:] == FC.PAD_ID).all() and (want[0][2, 5:] == -np.inf).all()
    assert want[2][3] == 0 and (want[1][3] == FC.PAD_ID).all()
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, tags=tags, any=any_, none=none_, exclude=ex)
    job = dict(world=2, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(x) for x in bounds], k=k)
    _check_ranks(launch(WORKER, tmp, 2, job), want)


def test_filtered_topk_with_an_empty_shard(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.quarter_set(52, 3, 2, 16)
    bounds = shard_bounds(2, 3)
    assert bounds == [(0, 1), (1, 2), (2, 2)]                    # rank 2 holds nothing
    tags = np.array([FC.bit(0), FC.bit(1)], np.uint64)
    any_ = np.array([FC.bit(0), FC.bit(0) | FC.bit(1), FC.bit(2)], np.uint64)
    none_ = np.zeros(3, np.uint64)
    ex = np.full((3, 1), -1, np.int64)
    k = 4                                                        # more than the index has rows
    want = _single_handle(q, t, tags, any_, none_, ex, k)
    assert want[2].tolist() == [1, 2, 0]
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, tags=tags, any=any_, none=none_, exclude=ex)
    job = dict(world=3, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(x) for x in bounds], k=k)
    _check_ranks(launch(WORKER, tmp, 3, job), want)
