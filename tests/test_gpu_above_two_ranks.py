"""ShardedIndex.score_above / count_above as REAL ranks: processes on the one GPU of a test box, a `gloo` group between them
(host-staged collectives), each holding its rows only.  Two ranks over uneven shards (4099 rows: 2050 + 2049) with an exact tie
across the boundary and another between far rows of the two shards, and three ranks over a two-row index (rank 2 holds
nothing); the result on EVERY rank must equal the single-handle score_above of the whole index.  One launch of
tests/above_two_rank_worker.py per rank; a child that fails, or the cap, ends the launch and the other children are killed; a
child that died of a signal ends the pytest session -- nothing more starts on the GPU after a fault."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import above_cases as AC
from tests import rank_cases as RC
from tests.util import make_pair, model_params
from tests.rank_launch import free_port, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "above_two_rank_worker.py")


def _single_handle(q, t, pair_q, thr):
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    m.handle.index_upload(t)
    want = m.handle.score_above(q, thr, pair_q)
    m.handle.close()
    AC.assert_above_equal(want, AC.expected_above(O.scores_f64(q, t.astype(np.float64)), pair_q, thr))
    return want


def _check_ranks(out, want, Q):
    for r in range(len(out)):
        AC.assert_above_equal((out[r]["offsets"], out[r]["ids"], out[r]["scores"]), want)
        assert np.array_equal(out[r]["counts"], np.diff(want[0])), "rank %d" % r
        assert str(out[r]["bad_q"]).startswith("ValueError")
        assert out[r]["empty_offsets"].tolist() == [0] and int(out[r]["empty_n"]) == 0
        assert int(out[r]["bruteforce"]) == 0


def test_score_above_on_two_ranks_equals_the_single_handle(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.shard_case()                                       # multiples of 1/4: exact in any order; row 4000 == row 10
    N, Q = t.shape[0], q.shape[0]
    bounds = shard_bounds(N, 2)
    assert bounds == [(0, 2050), (2050, 4099)]                   # uneven
    cut = bounds[1][0]
    t[cut] = t[cut - 1]                                          # a tie across the boundary itself
    sc = O.scores_f64(q, t.astype(np.float64))
    # per query: the score of the boundary rows, of rows 10 / 4000, a high cut, and thresholds nothing / everything passes
    thr = np.concatenate([sc[:, cut], sc[:, 10], np.quantile(sc, 0.98, axis=1), np.full(Q, np.inf), np.full(2, -np.inf)])
    pair_q = np.concatenate([np.tile(np.arange(Q, dtype=np.int32), 4), np.array([0, 1], np.int32)])
    want = _single_handle(q, t, pair_q, thr)
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, pair_q=pair_q, pair_thr=thr)
    job = dict(world=2, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(b) for b in bounds])
    out = launch(WORKER, tmp, 2, job)
    _check_ranks(out, want, Q)
    for p in range(Q):                                           # adjacent ids, equal scores, either side of the cut: consecutive
        seg = want[1][want[0][p]:want[0][p + 1]].tolist()
        assert seg.index(cut) == seg.index(cut - 1) + 1


def test_score_above_with_an_empty_shard(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.quarter_set(52, 3, 2, 16)
    bounds = shard_bounds(2, 3)
    assert bounds == [(0, 1), (1, 2), (2, 2)]                    # rank 2 holds nothing
    sc = O.scores_f64(q, t.astype(np.float64))
    thr = np.concatenate([sc.min(1), sc.max(1), np.full(3, np.inf)])
    pair_q = np.tile(np.arange(3, dtype=np.int32), 3)
    want = _single_handle(q, t, pair_q, thr)
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, pair_q=pair_q, pair_thr=thr)
    job = dict(world=3, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(b) for b in bounds])
    _check_ranks(launch(WORKER, tmp, 3, job), want, 3)
