"""ShardedIndex.rank_of as two REAL ranks: 2 processes on the one GPU of a test box, a `gloo` group between them (host-staged
collectives), each holding its rows only.  Uneven shards (4099 rows: 2050 + 2049), an exact tie across the boundary and
another between far rows of the two shards; the result on BOTH ranks must equal the single-handle score_rank of the whole
index.  One launch of tests/rank_two_rank_worker.py per rank; a child that fails, or the cap, ends the launch and the other
child is killed; a child that died of a signal ends the pytest session -- nothing more starts on the GPU after a fault."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import rank_cases as RC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "rank_two_rank_worker.py")
LAUNCH_CAP_S = 120                      # safety limit of the launch, not a measurement
FAULT_CODES = (134, 139, 124, 137)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tail(path, n=25):
    try:
        with open(path, errors="replace") as f:
            return "".join(f.readlines()[-n:])
    except OSError:
        return "(no output)"


def _launch(tmp, world, job):
    job_path = os.path.join(tmp, "job.json")
    with open(job_path, "w") as f:
        json.dump(job, f)
    procs, logs = [], []
    for r in range(world):
        logs.append((os.path.join(tmp, "rank%d.out" % r), os.path.join(tmp, "rank%d.err" % r)))
        with open(logs[r][0], "w") as fo, open(logs[r][1], "w") as fe:
            procs.append(subprocess.Popen([sys.executable, WORKER, job_path, str(r)], stdout=fo, stderr=fe,
                                          stdin=subprocess.DEVNULL, cwd=os.path.dirname(HERE)))
    deadline = time.monotonic() + LAUNCH_CAP_S
    ended, why = {}, None
    while len(ended) < world and why is None:
        for r, p in enumerate(procs):
            if r not in ended and p.poll() is not None:
                ended[r] = p.returncode
                if p.returncode != 0:
                    why = "rank %d ended with code %d" % (r, p.returncode)
        if why is None and len(ended) < world:
            if time.monotonic() > deadline:
                why = "no result after %d s" % LAUNCH_CAP_S
            else:
                time.sleep(0.1)
    for p in procs:                                              # nothing is left running, whatever happened
        if p.poll() is None:
            p.kill()
    for p in procs:
        p.wait()
    if why is not None:
        text = "launch of %d ranks: %s\n" % (world, why) + "".join(
            "---- rank %d (%s) stderr:\n%s---- stdout:\n%s" % (r, ended.get(r, "killed"), _tail(logs[r][1]), _tail(logs[r][0], 5))
            for r in range(world))
        if any(rc < 0 or rc in FAULT_CODES for rc in ended.values()):
            pytest.exit("a rank died of a signal; nothing more is started on the GPU\n" + text, returncode=3)
        pytest.fail(text, pytrace=False)
    return [np.load(os.path.join(tmp, "rank%d.npz" % r)) for r in range(world)]


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
    job = dict(world=2, port=_free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, bounds=[list(b) for b in bounds])
    out = _launch(tmp, 2, job)
    for r in range(2):
        assert np.array_equal(out[r]["ranks"], want), "rank %d" % r
        assert str(out[r]["bad_id"]).startswith("ValueError")
        assert out[r]["empty"].shape == (0,)
        assert int(out[r]["bruteforce"]) == 0
    i_lo, i_hi = np.flatnonzero(pair_id == cut - 1), np.flatnonzero(pair_id == cut)
    assert (want[i_hi] == want[i_lo] + 1).all()                  # adjacent ids, equal scores: consecutive ranks
