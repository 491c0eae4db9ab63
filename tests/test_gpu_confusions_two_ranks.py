"""ShardedIndex.score_confusions as REAL ranks: two processes on the one GPU of a test box, a `gloo` group between them
(host-staged collectives), each holding its rows only and both the same GLOBAL positives.  Uneven shards (4099 rows: 2050 +
2049, id_base 2050 on rank 1); an exact tie across the boundary whose rows sit on the floor of query 0 (its positive is their
copy on rank 1, margin 0); positives on rank 0 only, on rank 1 only, on both, on none; margins 0, 2.5 and +inf.  The result on
EVERY rank must equal the single-handle call on the whole index bit for bit -- lists, counts, best positive and the
(-inf, INT64_MAX) padding -- and that call the float64 oracle (scores exact in any order: the quarter construction).  One launch
of tests/confusions_two_rank_worker.py per rank (tests/rank_launch.py)."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import rank_cases as RC
from tests.util import make_pair, model_params
from tests.rank_launch import free_port, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "confusions_two_rank_worker.py")
PAD = np.iinfo(np.int64).max
MARGINS = (0.0, 2.5, float("inf"))


def _oracle(q, t, pos, margin, k):
    s = O.scores_f64(q, t.astype(np.float64))
    Q, N = s.shape
    ws, wi, wc = np.full((Q, k), -np.inf), np.full((Q, k), PAD, np.int64), np.zeros(Q, np.int32)
    wm, wb = np.full(Q, -np.inf), np.full(Q, PAD, np.int64)
    for qi in range(Q):
        rows = np.unique(pos[qi][(pos[qi] >= 0) & (pos[qi] < N)])
        ok = np.ones(N, bool)
        ok[rows] = False
        if rows.size:
            j = np.lexsort((rows, -s[qi, rows]))[0]
            wm[qi], wb[qi] = s[qi, rows[j]], rows[j]
        cols = np.flatnonzero(ok & (s[qi] >= wm[qi] - margin))
        c = min(k, cols.size)
        if c:
            ss, ii = O.topk(s[qi:qi + 1, cols], c)
            ws[qi, :c], wi[qi, :c], wc[qi] = ss[0], cols[ii[0]], c
    return ws, wi, wc, wm, wb


def test_confusions_on_two_ranks_equal_the_single_handle(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.shard_case()                                       # multiples of 1/4: exact in any order
    N, Q, k = t.shape[0], q.shape[0], 8
    bounds = shard_bounds(N, 2)
    assert bounds == [(0, 2050), (2050, 4099)]                   # uneven; rank 1's id_base is 2050
    cut = bounds[1][0]
    b = int(np.argmax((t.astype(np.float64) ** 2).sum(1)))       # the row of largest norm: it and its copies are the strict
    assert b > cut                                               # maxima of the query equal to it (Cauchy-Schwarz)
    t[cut - 1] = t[cut] = t[b]                                   # a tie across the boundary itself
    q[0] = t[b]
    s = O.scores_f64(q, t.astype(np.float64))
    o = np.argsort(-s, axis=1, kind="stable").astype(np.int64)
    pos = np.full((Q, 3), -1, np.int64)
    pos[0, 1] = b                                                # the two boundary rows score exactly m: on the floor
    for qi in range(1, Q):
        lo, hi = o[qi][o[qi] < cut], o[qi][o[qi] >= cut]
        if qi % 4 == 0:
            pos[qi] = [lo[3], -1, lo[20]]                        # rank 0 only
        elif qi % 4 == 1:
            pos[qi] = [hi[2], hi[2], N + 7]                      # rank 1 only, twice, and an id outside the index
        elif qi % 4 == 2:
            pos[qi] = [lo[30], hi[5], -1]                        # both: the best is rank 1's
        # qi % 4 == 3: no positive on any shard
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    h = m.handle
    h.index_upload(t)
    want = []
    for margin in MARGINS:
        got = h.score_confusions(q, k, pos, margin)
        for a, w in zip(got, _oracle(q, t, pos, margin, k)):
            assert np.array_equal(a, w), margin
        want.append(got)
    h.close()
    assert want[0][1][0, :2].tolist() == [cut - 1, cut] and want[0][2][0] == 2 and want[0][4][0] == b
    assert (want[2][2] == k).all() and (want[0][4][3::4] == PAD).all() and (want[0][2][3::4] == k).all()
    assert (want[0][2] < k).any() and (want[1][2] > want[0][2]).any()
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, pos=pos)
    job = dict(world=2, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(x) for x in bounds], k=k,
               margins=[repr(x) for x in MARGINS])
    out = launch(WORKER, tmp, 2, job)
    for r in range(2):
        for i in range(len(MARGINS)):
            for name, w in zip(("scores", "ids", "counts", "pos_scores", "pos_ids"), want[i]):
                a = out[r]["%s%d" % (name, i)]
                assert a.dtype == w.dtype and np.array_equal(a, w), "rank %d margin %r %s" % (r, MARGINS[i], name)
        assert str(out[r]["bad_k"]).startswith("ValueError") and str(out[r]["bad_margin"]).startswith("ValueError")
        assert int(out[r]["bruteforce"]) == 0
