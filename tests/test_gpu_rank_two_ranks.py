"""ShardedIndex.rank_of as two REAL ranks: 2 processes on the one GPU of a test box, a `gloo` group between them (host-staged
collectives), each holding its rows only.  Uneven shards (4099 rows: 2050 + 2049), an exact tie across the boundary and
another between far rows of the two shards; the result on BOTH ranks must equal the single-handle score_rank of the whole
index.  One launch of tests/rank_two_rank_worker.py per rank; a child that fails, or the cap, ends the launch and the other
child is killed; a child that died of a signal ends the pytest session -- nothing more starts on the GPU after a fault."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import rank_cases as RC
from tests.util import make_pair, model_params
from tests.rank_launch import free_port, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "rank_two_rank_worker.py")


def test_rank_of_on_two_ranks_equals_the_single_handle(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    q, t = RC.shard_case()                                       # multiples of 1/4: exact in any order; row 4000 == row 10
    N, Q = t.shape[0], q.shape[0]
    bounds = shard_bounds(N, 2)
    assert bounds == [(0, 2050), (2050, 4099)]                   # uneven
    cut = bounds[1][0]
    t[cut] = t[cut - 1]                                          # a tie across the boundary itself
    rng = np.random.RandomState(5)
    rows = np.unique(np.concatenate([rng.choice(N, size=300, replace=False), [0, 10, cut - 1, cut, 4000, N - 1]])).astype(np.int64)
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), len(rows))
    pair_id = np.tile(rows, Q)
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    m.handle.index_upload(t)
    want, _ = m.handle.score_rank(q, pair_q, pair_id)
    m.handle.close()
    assert np.array_equal(want, RC.ranks_from_scores(O.scores_f64(q, t.astype(np.float64)))[pair_q, pair_id])
    sc = O.scores_f64(q, t.astype(np.float64))
    assert (sc[:, cut] == sc[:, cut - 1]).all()
    np.savez(os.path.join(tmp, "inputs.npz"), t=t, q=q, pair_q=pair_q, pair_id=pair_id)
    job = dict(world=2, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(b) for b in bounds])
    out = launch(WORKER, tmp, 2, job)
    for r in range(2):
        assert np.array_equal(out[r]["ranks"], want), "rank %d" % r
        assert str(out[r]["bad_id"]).startswith("ValueError")
        assert out[r]["empty"].shape == (0,)
        assert int(out[r]["bruteforce"]) == 0
    i_lo, i_hi = np.flatnonzero(pair_id == cut - 1), np.flatnonzero(pair_id == cut)
    assert (want[i_hi] == want[i_lo] + 1).all()                  # adjacent ids, equal scores: consecutive ranks
