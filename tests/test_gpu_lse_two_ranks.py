"""ShardedIndex.score_lse as REAL ranks: two processes on the one GPU of a test box, a `gloo` group between them (host-staged
collectives), each holding its rows, tag words and bias values only.  Uneven shards (1201 rows: 601 + 600, id_base 601 on
rank 1), tags and bias set per shard, one query whose eligible rows all live on rank 1, one with none anywhere, one
unrestricted, a weight per query.  Both ranks must hold the same (lse, count, bound) bit for bit, and it must pass
lse_cases.check() against the float64 reference of the WHOLE index.  One launch of tests/lse_two_rank_worker.py per rank, each
under its own time limit; a child that fails ends the launch and the other child is killed; a child that died of a signal ends
the pytest session -- nothing more starts on the GPU after a fault."""
import os

import numpy as np
import pytest

from tests import lse_cases as LC
from tests.rank_launch import free_port, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "lse_two_rank_worker.py")


CUT = 601


def _tags(case, rng):
    """lse_cases._t_mixed (query 0: nothing eligible, query 1: unrestricted, query 2: the last row alone) with bit 30 on forty
    rows of rank 1 only, which query 3 asks for"""
    d = LC._t_mixed(case, rng)
    rows = CUT + rng.choice(case.N - CUT - 1, 40, replace=False)
    d["tags"][rows] |= LC.bit(30)
    d["any"][3], d["none"][3] = LC.bit(30), 0
    return d


CASE = LC.Case("two_ranks", 9, 1201, 40, 64, 31, tags=_tags, bias=LC._b_mixed, why="uneven shards, tags and bias per shard")
PLAIN = LC.Case("two_ranks_plain", 9, 1201, 40, 64, 31, why="the same rows and queries without masks and bias")


def test_lse_on_two_ranks_passes_the_check_of_the_whole_index(tmp_path):
    from sse_amd.sharded import shard_bounds
    tmp = str(tmp_path)
    I = LC.inputs(CASE)
    bounds = shard_bounds(CASE.N, 2)
    assert bounds == [(0, CUT), (CUT, 1201)]                     # uneven; id_base = 601 on rank 1
    e = LC.eligible(CASE)
    want, wc = LC.reference(CASE)
    assert wc[0] == 0 and wc[2] == 1 and e[2, CASE.N - 1]
    assert wc[3] == 40 and not e[3, :CUT].any()                  # every eligible row of query 3 on rank 1
    assert e[1, :CUT].any() and e[1, CUT:].any() and I["any"][1] == 0
    assert np.array_equal(LC.inputs(PLAIN)["q"], I["q"]) and np.array_equal(LC.inputs(PLAIN)["t"], I["t"])
    np.savez(os.path.join(tmp, "inputs.npz"), t=I["t"], q=I["q"], tags=I["tags"], any=I["any"], none=I["none"], bias=I["bias"], w=I["w"])
    job = dict(world=2, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(x) for x in bounds],
               scale=CASE.scale)
    out = launch(WORKER, tmp, 2, job)
    for key in ("lse", "count", "bound", "plain_lse", "plain_count", "plain_bound"):
        assert out[0][key].tobytes() == out[1][key].tobytes(), key
    for r in range(2):
        used, over = LC.check(CASE, out[r]["lse"], out[r]["count"], out[r]["bound"])
        LC.check(PLAIN, out[r]["plain_lse"], out[r]["plain_count"], out[r]["plain_bound"])
        assert str(out[r]["bad_len"]).startswith("ValueError")
        assert int(out[r]["id_base_local_calls"]) == 2
    print("LSER two ranks: worst |lse - ref| = %.4f of the bound, bound - d_q <= %.3e" % (used, over))
