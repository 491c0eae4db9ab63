"""ShardedIndex.score_topk_grouped as REAL ranks: processes on the one GPU of a test box, a `gloo` group between them
(host-staged collectives), each holding its rows, group keys and tag words only.  Two ranks over uneven shards (4099 rows: 2050
+ 2049) with a group whose best row is on rank 1 and whose second-best row is inside rank 0's local top-k (the merge must drop
it), an exact tie across the boundary between rows of different groups, groups living on rank 1 only, a query with fewer than
k groups in total (two of them spanning both ranks), one with no eligible row; three ranks over a two-row index (rank 2 holds
nothing, k exceeds the rows, both rows one group).  The result on EVERY rank must equal the single-handle call on the whole
index, and that the float64 reference.  One launch of tests/grouped_two_rank_worker.py per rank; a child that fails, or the cap,
ends the launch and the other children are killed; a child that died of a signal ends the pytest session -- nothing more
starts on the GPU after a fault."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import grouped_cases as GC
from tests.filtered_cases import U1, bit
from tests import rank_cases as RC
from tests.util import make_pair, model_params
from tests.rank_launch import free_port, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "grouped_two_rank_worker.py")


def _reference(q, t, groups, tags, any_, none_, k):
    """the float64 oracle of the whole index (scores exact in any order: the quarter construction)"""
    s = O.scores_f64(q, t.astype(np.float64))
    Q, N = s.shape
    e = ((any_[:, None] == 0) | ((tags[None, :] & any_[:, None]) != 0)) & ((tags[None, :] & none_[:, None]) == 0)
    ws, wi, wg, wc = np.full((Q, k), -np.inf), np.full((Q, k), GC.PAD, np.int64), np.full((Q, k), GC.PAD, np.int64), np.zeros(Q, np.int32)
    for qi in range(Q):
        cols = np.flatnonzero(e[qi])
        if not cols.size:
            continue
        _, ii = O.topk(s[qi:qi + 1, cols], cols.size)
        reps = GC.collapse(cols[ii[0]], groups)[:k]
        c = reps.size
        ws[qi, :c], wi[qi, :c], wg[qi, :c], wc[qi] = s[qi, reps], reps, groups[reps], c
    return ws, wi, wg, wc


def _single_handle(q, t, groups, tags, any_, none_, k):
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    m.handle.index_upload(t)
    m.handle.index_set_groups(groups)
    m.handle.index_set_tags(tags)
    want = m.handle.score_topk_grouped(q, k, any_of=any_, none_of=none_)
    m.handle.close()
    ref = _reference(q, t, groups, tags, any_, none_, k)
    for a, b in zip(want, ref):
        assert np.array_equal(a, b)
    return want


def _check_ranks(out, want):
    for r in range(len(out)):
        assert np.array_equal(out[r]["ids"], want[1]), "rank %d" % r
        assert np.array_equal(out[r]["scores"], want[0]), "rank %d" % r
        assert np.array_equal(out[r]["groups"], want[2]), "rank %d" % r
        assert np.array_equal(out[r]["counts"], want[3]) and out[r]["counts"].dtype == np.int32, "rank %d" % r
        assert str(out[r]["bad_k"]).startswith("ValueError")
        assert int(out[r]["bruteforce"]) == 0


def test_grouped_topk_on_two_ranks_equals_the_single_handle(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.shard_case()                                       # multiples of 1/4: exact in any order
    N, Q, k = t.shape[0], q.shape[0], 8
    bounds = shard_bounds(N, 2)
    assert bounds == [(0, 2050), (2050, 4099)]                   # uneven
    cut = bounds[1][0]
    b = int(np.argmax((t.astype(np.float64) ** 2).sum(1)))       # the row of largest norm: it and its copies are the strict
    assert b not in (cut - 1, cut)                               # maxima of the query equal to it (Cauchy-Schwarz)
    t[cut - 1] = t[cut] = t[b]                                   # a tie across the boundary itself
    q[0] = t[b]
    rng = np.random.RandomState(7)
    groups = rng.randint(0, 1000, size=N).astype(np.int64) * 3 - 1500       # ~4 rows each, on either rank
    groups[[b, cut - 1, cut]] = [10 ** 12, 10 ** 12 + 1, -10 ** 12]          # the tied rows: three groups
    tags = (bit(0) | (U1 << rng.randint(1, 4, size=N).astype(np.uint64))).astype(np.uint64)
    only1 = rng.choice(np.arange(cut + 1, N - 1), 30, replace=False)
    tags[only1] |= bit(5)                                                    # rank 1 only ...
    groups[only1] = 2 * 10 ** 12 + np.arange(30) // 3                        # ... in ten groups that live there
    tags[[5, 700, 2049, 2051, 4098]] |= bit(6)                               # five rows, three groups, two of them on both ranks
    groups[[5, 2051]] = 3 * 10 ** 12
    groups[[700, 4098]] = GC.PAD                                             # (a real group with the padding key)
    groups[2049] = GC.I64_MIN
    any_ = (U1 << rng.randint(0, 4, size=Q).astype(np.uint64)).astype(np.uint64)
    any_[0], any_[1], any_[2], any_[3], any_[4], any_[5] = bit(0), bit(5), bit(6), bit(7), np.uint64(0), np.uint64(0)
    none_ = np.zeros(Q, np.uint64)
    none_[6:] = bit(3)
    # query 5: the best row of rank 1 and the best lower-scoring row of rank 0 share a group
    s = O.scores_f64(q, t.astype(np.float64))
    special = set([b, cut - 1, cut, 5, 700, 2049, 2051, 4098] + only1.tolist())
    r1 = cut + int(np.argmax(s[5, cut:]))
    r0 = next(int(r) for r in np.argsort(-s[5, :cut], kind="stable") if s[5, r] < s[5, r1])
    assert r0 not in special and r1 not in special
    groups[[r0, r1]] = 4 * 10 ** 12
    local0 = _reference(q, t[:cut], groups[:cut], tags[:cut], any_, none_, k)
    assert r0 in local0[1][5].tolist()                           # rank 0 sends it ...
    want = _single_handle(q, t, groups, tags, any_, none_, k)
    assert r1 in want[1][5].tolist() and r0 not in want[1][5].tolist() and want[2][5].tolist().count(4 * 10 ** 12) == 1   # ... the merge drops it
    assert want[1][0, :3].tolist() == sorted([b, cut - 1, cut]) and want[0][0, 0] == want[0][0, 2]
    assert len(set(want[2][0, :3].tolist())) == 3
    assert (want[1][1, :k] >= cut).all() and want[3][1] == k and (want[2][1] >= 2 * 10 ** 12).all()   # groups of rank 1 only
    assert want[3][2] == 3 and (want[1][2, 3:] == GC.PAD).all() and (want[0][2, 3:] == -np.inf).all()
    assert sorted(want[2][2, :3].tolist()) == [GC.I64_MIN, 3 * 10 ** 12, GC.PAD]
    assert want[3][3] == 0 and (want[1][3] == GC.PAD).all()
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, groups=groups, tags=tags, any=any_, none=none_)
    job = dict(world=2, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(x) for x in bounds], k=k)
    _check_ranks(launch(WORKER, tmp, 2, job), want)


def test_grouped_topk_with_an_empty_shard(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.quarter_set(52, 3, 2, 16)
    bounds = shard_bounds(2, 3)
    assert bounds == [(0, 1), (1, 2), (2, 2)]                    # rank 2 holds nothing
    groups = np.array([-9, -9], np.int64)                        # one group over ranks 0 and 1
    tags = np.array([bit(0), bit(1)], np.uint64)
    any_ = np.array([bit(0), bit(0) | bit(1), bit(2)], np.uint64)
    none_ = np.zeros(3, np.uint64)
    k = 4                                                        # more than the index has rows
    want = _single_handle(q, t, groups, tags, any_, none_, k)
    assert want[3].tolist() == [1, 1, 0]
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, groups=groups, tags=tags, any=any_, none=none_)
    job = dict(world=3, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(x) for x in bounds], k=k)
    _check_ranks(launch(WORKER, tmp, 3, job), want)
