"""sse_score_rank*: the exact 0-based rank of labelled rows over the whole resident index -- the position a row would have in
sse_score_topk(..., k = N) -- against the ranking the library already certifies (score_topk), the CPU oracle, exact-tie and
near-tie constructions (tests/rank_cases.py; proven exact in tests/test_rank_metrics_host.py), row shards through thresholds,
the device-pointer form and the error paths.  Bar: ranks equal, scores the same 64 bits as score_topk's."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import rank_cases as RC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

BRUTE, BAND = "score_rank_bruteforce_pairs", "score_rank_band_rows"


def _scorer(S=8):
    params = model_params("dual-encoder", 50, 8, 16, 16, S, 4)
    m, _ = make_pair(params)
    return m.handle


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _check_against_topk(h, q, N, k):
    """for every (query, j): the row score_topk ranks j-th has rank j and the same score bits"""
    k = min(k, N)
    sc, ids = h.score_topk(q, k)
    Q = q.shape[0]
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), k)
    brute0 = h.get_counter(BRUTE)
    before, score = h.score_rank(q, pair_q, ids.reshape(-1))
    assert np.array_equal(before.reshape(Q, k), np.broadcast_to(np.arange(k), (Q, k)))
    assert np.array_equal(_bits(score), _bits(sc.reshape(-1)))
    assert h.get_counter(BRUTE) == brute0


@pytest.mark.parametrize("Q,N,S,how", [(257, 4099, 256, "f32"), (257, 4099, 256, "f64"), (257, 4099, 256, "dev"),
                                       (257, 31, 50, "f32"), (257, 31, 50, "f64"), (257, 31, 50, "dev"),
                                       (33, 1, 50, "f32"), (33, 1, 256, "f64"), (33, 1, 256, "dev"),
                                       (40, 700, 300, "f32"), (40, 700, 620, "f32"), (8, 8227, 20, "f32")])
def test_rank_agrees_with_certified_topk(Q, N, S, how):
    """N = 4099: a partial last tile and 8 index splits; S = 50: not a multiple of 8; N = 1.  Index uploaded as float32, as
    float64 (the re-scorer then reads the float64 rows) and adopted from device memory.
    The sweep's other instantiations and its other decode (csrc/score_sweep.h): S = 300 (296 < S <= 616) is two pair tiles
    per workgroup, S = 620 one, with 78 k-groups (78 % 4 = 2: the head of the k-loop and its ring); the 2560 pairs leave the
    last pair block partial.  N = 8227 = 257 * 32 + 3 is 258 tiles with a partial last one, and choose_nsplit gives 16 splits
    for any number of pairs: doubling goes on while 258 / (2 splits) >= 16, so it stops at 16, and evening out the rounds
    needs 200 tiles per split.  More than 8 splits is the second branch of the workgroup decode and of the grid size;
    S = 20 is 3 k-groups: all head, no ring body."""
    rng = np.random.RandomState(Q + N + S)
    q, t = RC.unit(rng, Q, S), RC.unit(rng, N, S)
    h = _scorer()
    if how == "f32":
        h.index_upload(t)
    elif how == "f64":
        t64 = RC.unit(rng, N, S).astype(np.float64) * (1.0 + 1e-9)     # values that are NOT float32 numbers
        h.index_upload(t64)
    else:
        import torch
        rows = torch.from_numpy(t).to("cuda:0")
        h.index_set_dev(rows.data_ptr(), N, S)
        torch.cuda.synchronize()
    _check_against_topk(h, q, N, 64)


def test_rank_of_every_row_against_oracle():
    Q, N, S = 33, 571, 64
    rng = np.random.RandomState(7)
    q, t = RC.unit(rng, Q, S), RC.unit(rng, N, S)
    scores = O.scores_f64(q, t.astype(np.float64))
    ssc, _ = O.sorted_results(scores)
    gap = float(np.min(ssc[:, :-1] - ssc[:, 1:]))
    assert gap > 1e-9, gap            # no near-tie can decide this case silently (summation orders differ by ~1e-16)
    want = RC.ranks_from_scores(scores)
    h = _scorer()
    h.index_upload(t)
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), N)
    pair_id = np.tile(np.arange(N, dtype=np.int64), Q)
    brute0 = h.get_counter(BRUTE)
    before, score = h.score_rank(q, pair_q, pair_id)
    assert np.array_equal(before.reshape(Q, N), want)
    assert np.abs(score.reshape(Q, N) - scores).max() < 1e-12
    assert h.get_counter(BRUTE) == brute0


def test_exact_ties_rank_in_id_order():
    q, t, copies = RC.exact_ties_case()
    Q, N = q.shape[0], t.shape[0]
    want = RC.ranks_from_scores(O.scores_f64(q, t.astype(np.float64)))
    h = _scorer()
    h.index_upload(t)
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), N)
    pair_id = np.tile(np.arange(N, dtype=np.int64), Q)
    brute0 = h.get_counter(BRUTE)
    before, _ = h.score_rank(q, pair_q, pair_id)
    before = before.reshape(Q, N)
    assert np.array_equal(before, want)
    assert before[0, copies].tolist() == list(range(len(copies)))      # the 31 maxima of query 0: consecutive, in id order
    sc = O.scores_f64(q, t.astype(np.float64))
    between = (sc[:, 4:N - 1] == sc[:, 3:4]).sum(1)                    # other rows that tie with row 3 exactly
    assert (before[:, N - 1] == before[:, 3] + 1 + between).all()      # a copy ranks behind its original and the ties between
    assert h.get_counter(BRUTE) == brute0


def _near_tie_labels(t, where, n_generic, rng):
    far = np.flatnonzero(np.abs(t[:, 0] - 0.5) > 1e-3)                 # generic rows nowhere near the cluster's band
    return where, rng.choice(far, size=n_generic, replace=False)


def test_near_ties_below_fp32_resolution():
    q, t, where = RC.near_tie_case(200, 1000)
    want = RC.ranks_from_scores(O.scores_f64(q, t))
    rng = np.random.RandomState(1)
    cl, gen = _near_tie_labels(t, where, 50, rng)
    ids = np.concatenate([cl, gen]).astype(np.int64)
    pair_q = np.repeat(np.arange(2, dtype=np.int32), len(ids))
    pair_id = np.tile(ids, 2)
    h = _scorer()
    h.index_upload(t)
    band0, brute0 = h.get_counter(BAND), h.get_counter(BRUTE)
    before, score = h.score_rank(q, pair_q, pair_id)
    assert np.array_equal(before, want[pair_q, pair_id])
    assert np.array_equal(_bits(score), _bits(O.scores_f64(q, t)[pair_q, pair_id]))   # one product per score: exact
    assert h.get_counter(BAND) - band0 >= 200
    assert h.get_counter(BRUTE) == brute0


def test_band_overflow_is_counted_in_float64():
    q, t, where = RC.near_tie_case(5000, 6000)
    want = RC.ranks_from_scores(O.scores_f64(q, t))
    rng = np.random.RandomState(2)
    cl, gen = _near_tie_labels(t, where, 20, rng)
    cl = cl[rng.choice(len(cl), size=40, replace=False)]
    ids = np.concatenate([cl, gen]).astype(np.int64)
    pair_q = np.repeat(np.arange(2, dtype=np.int32), len(ids))
    pair_id = np.tile(ids, 2)
    h = _scorer()
    h.index_upload(t)
    brute0 = h.get_counter(BRUTE)
    before, _ = h.score_rank(q, pair_q, pair_id)
    assert np.array_equal(before, want[pair_q, pair_id])
    assert h.get_counter(BRUTE) - brute0 == 2 * len(cl)                # 5000 rows in the band of every cluster label > 4096


def test_shards_add_through_thresholds():
    q, t = RC.shard_case()
    Q, N = q.shape[0], t.shape[0]
    cut = 2000
    rng = np.random.RandomState(3)
    rows = np.unique(np.concatenate([rng.choice(N, size=400, replace=False), [0, 10, cut - 1, cut, 4000, N - 1]])).astype(np.int64)
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), len(rows))
    pair_id = np.tile(rows, Q)
    h = _scorer()
    brute0 = h.get_counter(BRUTE)
    h.index_upload(t)
    whole, whole_sc = h.score_rank(q, pair_q, pair_id)
    assert np.array_equal(whole, RC.ranks_from_scores(O.scores_f64(q, t.astype(np.float64)))[pair_q, pair_id])
    owner = (pair_id >= cut).astype(int)
    parts = [(0, t[:cut]), (cut, t[cut:])]
    score = np.empty(len(pair_id), np.float64)
    total = np.zeros(len(pair_id), np.int64)
    for s, (base, shard) in enumerate(parts):                          # owned pairs: first form
        h.index_upload(shard, id_base=base)
        m = owner == s
        b, sc = h.score_rank(q, pair_q[m], pair_id[m])
        total[m] += b
        score[m] = sc
    for s, (base, shard) in enumerate(parts):                          # the other shard: thresholds
        h.index_upload(shard, id_base=base)
        m = owner != s
        b, _ = h.score_rank(q, pair_q[m], pair_id[m], pair_score=score[m])
        total[m] += b
    assert np.array_equal(_bits(score), _bits(whole_sc))
    assert np.array_equal(total, whole)
    i10, i4000 = np.flatnonzero(pair_id == 10), np.flatnonzero(pair_id == 4000)
    sc = O.scores_f64(q, t.astype(np.float64))
    between = (sc[:, 11:4000] == sc[:, 10:11]).sum(1)
    assert (whole[i4000] == whole[i10] + 1 + between).all()            # the tie across the cut: lower id first
    assert h.get_counter(BRUTE) == brute0


def test_dev_form_on_a_stream_equals_host_form():
    import torch
    Q, N, S = 65, 2049, 64
    rng = np.random.RandomState(9)
    q, t = RC.unit(rng, Q, S), RC.unit(rng, N, S)
    pair_q = rng.randint(0, Q, size=777).astype(np.int32)
    pair_id = rng.randint(0, N, size=777).astype(np.int64)
    h = _scorer()
    h.index_upload(t)
    brute0 = h.get_counter(BRUTE)
    want_b, want_s = h.score_rank(q, pair_q, pair_id)
    thr = want_s + rng.choice([0.0, 1e-3, -1e-3], size=777)
    want_b2, _ = h.score_rank(q, pair_q, pair_id + 5, pair_score=thr)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        dq, dpq, dpi = torch.from_numpy(q).to(dev), torch.from_numpy(pair_q).to(dev), torch.from_numpy(pair_id).to(dev)
        dpi2, dthr = torch.from_numpy(pair_id + 5).to(dev), torch.from_numpy(thr).to(dev)
        ob = torch.full((777,), -1, dtype=torch.int64, device=dev)
        osc = torch.full((777,), float("nan"), dtype=torch.float64, device=dev)
        ob2 = torch.full((777,), -1, dtype=torch.int64, device=dev)
        h.score_rank_dev(dq.data_ptr(), Q, dpq.data_ptr(), dpi.data_ptr(), 777, None, ob.data_ptr(), osc.data_ptr(), st.cuda_stream)
        h.score_rank_dev(dq.data_ptr(), Q, dpq.data_ptr(), dpi2.data_ptr(), 777, dthr.data_ptr(), ob2.data_ptr(), None, st.cuda_stream)
    st.synchronize()
    h.synchronize()
    assert np.array_equal(ob.cpu().numpy(), want_b)
    assert np.array_equal(_bits(osc.cpu().numpy()), _bits(want_s))
    assert np.array_equal(ob2.cpu().numpy(), want_b2)
    assert h.get_counter(BRUTE) == brute0


def test_errors_leave_outputs_untouched_and_the_handle_usable():
    import ctypes as C
    import sse_amd
    import torch
    Q, N, S = 4, 100, 16
    rng = np.random.RandomState(4)
    q, t = RC.unit(rng, Q, S), RC.unit(rng, N, S)
    h = _scorer()

    def raw(pair_q, pair_id):
        pq, pid = np.asarray(pair_q, np.int32), np.asarray(pair_id, np.int64)
        before, score = np.full(len(pq), -7, np.int64), np.full(len(pq), -7.0)
        rc = h.lib.sse_score_rank(h._h, q.ctypes.data_as(C.c_void_p), Q, pq.ctypes.data_as(C.c_void_p), pid.ctypes.data_as(C.c_void_p),
                                  len(pq), None, before.ctypes.data_as(C.c_void_p), score.ctypes.data_as(C.c_void_p))
        return rc, before, score, h.lib.sse_last_error(h._h).decode()

    rc, b, s, msg = raw([0, 1], [3, 4])                                # no index set
    assert rc != 0 and "index" in msg and (b == -7).all() and (s == -7.0).all()
    h.index_upload(t, id_base=1000)
    for pq, pid, word in (([0, 1, 2], [1000, 1100, 1001], "pair_id"), ([0, 1], [999, 1001], "pair_id"),
                          ([0, Q], [1000, 1001], "pair_q"), ([-1, 0], [1000, 1001], "pair_q")):
        rc, b, s, msg = raw(pq, pid)
        assert rc != 0 and word in msg, (rc, msg)
        assert (b == -7).all() and (s == -7.0).all()
        with pytest.raises(sse_amd.SSEError):
            h.score_rank(q, pq, pid)
    # second form: any id goes, a pair_q out of range does not
    b2, _ = h.score_rank(q, [0, 1], [-5, 2 ** 40], pair_score=[2.0, -2.0])
    assert b2.tolist() == [0, N]
    with pytest.raises(sse_amd.SSEError):
        h.score_rank(q, [0, Q], [0, 0], pair_score=[0.0, 0.0])
    # L = 0, then a valid call
    b0, s0 = h.score_rank(q, [], [])
    assert b0.shape == (0,) and s0.shape == (0,)
    want = RC.ranks_from_scores(O.scores_f64(q, t.astype(np.float64)))
    bv, _ = h.score_rank(q, [0, 1, 2, 3], [1000, 1050, 1099, 1001])
    assert bv.tolist() == [want[0, 0], want[1, 50], want[2, 99], want[3, 1]]
    # device form: a bad pair surfaces through synchronize(), nothing is written, the next call is served
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q).to(dev)
    dpq = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    dpi = torch.tensor([1000, 1100], dtype=torch.int64, device=dev)
    ob = torch.full((2,), -7, dtype=torch.int64, device=dev)
    osc = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    h.score_rank_dev(dq.data_ptr(), Q, dpq.data_ptr(), dpi.data_ptr(), 2, None, ob.data_ptr(), osc.data_ptr())
    with pytest.raises(sse_amd.SSEError):
        h.synchronize()
    assert ob.cpu().tolist() == [-7, -7] and osc.cpu().tolist() == [-7.0, -7.0]
    dpi = torch.tensor([1000, 1050], dtype=torch.int64, device=dev)
    h.score_rank_dev(dq.data_ptr(), Q, dpq.data_ptr(), dpi.data_ptr(), 2, None, ob.data_ptr(), osc.data_ptr())
    h.synchronize()
    assert ob.cpu().tolist() == [want[0, 0], want[1, 50]]
