"""The host read-back of sse_score_topk / sse_encode_score_topk (score_to_host_locked, csrc/sse_api.hip) with an encoder in
front of it and an open certificate behind it, in both of its forms: Q <= 64 polls the pinned mirror the re-scoring pass
stores through, Q > 64 takes copies, one synchronisation and the encoder's error flag riding along.

One small LSTM model, one index of N = 200 encodings of which COPIES = 40 are bit-equal copies of the encoding of pool row 0:
more than the 16 candidates of the one split such an index is swept in (choose_nsplit: 7 tiles).  A call whose query 0 IS
pool row 0 ("planted") has its k-th best score tied with rows outside the candidate list for every k <= 16: a bit-equal row
has a bit-equal fp32 score, so the bound of the rows left out is no smaller than the k-th candidate and the re-scoring pass
cannot certify the query -- the call needs its second stage (collect sweep + float64 select: 40 rows fit the collect buffer,
nothing goes to the brute force).  The other queries are encodings of rows the index does not hold.

Reference: O.topk(O.scores_f64(enc, t)) with enc = encode_source of the same ids in the same batch (the same kernel, bit-equal
to what sse_encode_score_topk scores).  The copies get ONE reference column, as in tests/topk_cases.py.  Ids bit-equal, ties
by lower row; scores within 1e-12 (the bar of tests/test_gpu_score.py: |q|, |t| <= 1)."""
import functools

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import make_pair, model_params, random_ids

pytestmark = pytest.mark.gpu

V, T, S, N, COPIES, QMAX = 300, 20, 64, 200, 40, 70
PARAMS = model_params("dual-encoder", V, 50, 96, 96, S, T)
SEED = 72
GROUP = np.r_[0, np.arange(5, N, 5)]          # rows 0, 5, 10 .. 195: the first tile, every tile, the last (partial) tile
EPS32 = 2.0 * (S + 2) * 5.97e-8               # score_eps32 of csrc/sse_api.hip per unit |q| |t|
COUNTERS = ("score_collect_queries", "score_bruteforce_queries", "score_bf16_second_chance_queries", "score_two_pass_calls")


def pool_ids(seed=SEED):
    """[N + QMAX] id rows: the first N are the index (row 0 is the copied one), the rest are the ordinary queries"""
    return random_ids(np.random.RandomState(seed), N + QMAX, T, V, 0.5)


def index_rows(enc_pool):
    t = np.array(enc_pool[:N], np.float32)
    t[GROUP] = t[0]
    t.setflags(write=False)
    return t


def query_ids(pool, Q, planted):
    """planted: pool row 0 and Q - 1 ordinary rows; else Q ordinary rows (the same ones in rows 1 .. Q - 1)"""
    ids = pool[N:N + Q].copy()
    if planted:
        ids[0] = pool[0]
    return ids


def reference(enc, t, k):
    """(scores [Q, k], ids [Q, k]) of O.topk over O.scores_f64, the copies sharing the original's column"""
    keep = np.ones(N, bool)
    keep[GROUP[1:]] = False
    col = np.cumsum(keep) - 1
    col[GROUP] = col[GROUP[0]]
    s = O.scores_f64(enc, t[keep].astype(np.float64))[:, col]
    return O.topk(s, k)


def preconditions(enc, t, k, planted):
    """AssertionError unless the reference is one a device summing in its own order must reproduce id for id (the style of
    topk_cases.preconditions), and unless the certificates come out as the counter claims need them."""
    Q = enc.shape[0]
    assert len(GROUP) == COPIES and COPIES > 16 and enc.shape == (Q, S) and t.shape == (N, S)
    tb = np.ascontiguousarray(t[GROUP])
    assert (tb.view(np.uint8) == tb[:1].view(np.uint8)).all(), "copies are not bit-equal rows"
    assert len({t[r].tobytes() for r in range(N)}) == N - COPIES + 1, "an unplanned duplicate row"
    qn = float(np.linalg.norm(enc.astype(np.float64), axis=1).max())
    tn = float(np.linalg.norm(t.astype(np.float64), axis=1).max())
    assert qn <= 1 + 1e-6 and tn <= 1 + 1e-6
    tol = 2.0 * S * 2.0 ** -53 * qn * tn         # two float64 sums of S products in different orders
    ws, wi = reference(enc, t, COPIES + 1)           # (k + 1 <= 18 and the 16 candidates lie inside)
    in_group = np.zeros(N, bool)
    in_group[GROUP] = True
    gap = (ws[:, :-1] - ws[:, 1:])[:, :k]
    both = (in_group[wi[:, :-1]] & in_group[wi[:, 1:]])[:, :k]
    assert (gap[both] == 0).all()
    assert gap[~both].min() > 2 * tol, "neighbours %.3e apart, 2 tol = %.3e" % (gap[~both].min(), 2 * tol)
    ordinary = np.arange(1 if planted else 0, Q)
    if planted:
        # the copies are the planted query's strict maxima: its list is the lowest copy rows
        n = min(k, COPIES)
        assert np.array_equal(wi[0, :n], GROUP[:n]) and ws[0, n - 1] - ws[0, COPIES] > 1e-3
    if k <= 16:
        # An ordinary query is certified.  rescore_kernel certifies when (largest bound of the rows left out) + eps32 |q| < exact
        # k-th candidate.  The bound of the one split is max(16th merged candidate, 8th entry of any full lane list)
        # (score_topk.hip, "Lists"): an fp32 score no larger than the 8th best row's, which is within eps32 |q| of that row's
        # exact score.  So k-th best - 8th best > 2 eps32 |q| |t|max closes the certificate -- and says that the 40 tied copies
        # are not at the query's k-th rank.
        assert k < 8
        margin = ws[ordinary, k - 1] - ws[ordinary, 7]
        assert margin.min() > 2 * EPS32 * qn * tn, "k-th and 8th best %.3e apart" % margin.min()
    return True


class World:
    def __init__(self):
        self.m, self.p = make_pair(PARAMS, seed=13)
        self.pool = pool_ids()
        self.t = index_rows(self.m.encode_source(self.pool[:N]))
        self.m.handle.index_upload(self.t)

    def counters(self):
        return {n: self.m.handle.get_counter(n) for n in COUNTERS}

    def moved(self, before):
        now = self.counters()
        return {n: now[n] - before[n] for n in COUNTERS}


@functools.lru_cache(maxsize=None)
def world():
    return World()


@functools.lru_cache(maxsize=None)
def encodings(Q, planted):
    """encode_source of the case's ids: the queries of the host form and of the reference; read-only"""
    w = world()
    enc = w.m.encode_source(query_ids(w.pool, Q, planted))
    enc.setflags(write=False)
    return enc


def check(got_s, got_i, enc, t, k):
    ws, wi = reference(enc, t, k)
    assert got_s.shape == ws.shape and got_s.dtype == np.float64 and got_i.dtype == np.int64
    assert np.array_equal(got_i, wi), "ids differ at %s" % (np.argwhere(got_i != wi)[:3].tolist(),)
    worst = float(np.abs(got_s - ws).max())
    print("max |score - reference| = %.3e" % worst)
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("planted", [True, False], ids=["planted", "plain"])
@pytest.mark.parametrize("k", [5, 17])
@pytest.mark.parametrize("Q", [5, 70])
@pytest.mark.parametrize("form", ["score_topk", "encode_score_topk"])
def test_read_back(form, Q, k, planted):
    w = world()
    h = w.m.handle
    ids = query_ids(w.pool, Q, planted)
    enc = encodings(Q, planted)
    assert preconditions(enc, w.t, k, planted)
    before = w.counters()
    if form == "score_topk":
        got_s, got_i = h.score_topk(enc, k)
    else:
        got_s, got_i = h.encode_score_topk(0, ids, True, k)
    moved = w.moved(before)
    print(form, Q, k, planted, moved)
    check(got_s, got_i, enc, w.t, k)
    assert moved["score_bruteforce_queries"] == 0 and moved["score_two_pass_calls"] == 0 and moved["score_bf16_second_chance_queries"] == 0
    if k > 16:
        assert moved["score_collect_queries"] == Q       # the select route serves every query (tests/topk_cases.py)
    elif planted:
        # Query 0 cannot be certified (module docstring) and its 40 tied rows fit a collect buffer: the select kernel serves it,
        # + 1.  The ordinary queries are certified by the margin of preconditions(); `>=` because that margin is an argument
        # about the reference's scores, the certificate is the kernel's own arithmetic.
        assert moved["score_collect_queries"] >= 1
    else:
        assert moved["score_collect_queries"] == 0       # every certificate closed: the second stage is not run


def test_bad_id_at_q70_raises_and_the_next_call_is_clean():
    """the error flag rides along with the copies of the first stage (Q > 64): nothing is returned, the next call is clean"""
    import sse_amd
    w = world()
    h = w.m.handle
    ids = query_ids(w.pool, 70, True)
    want_s, want_i = h.encode_score_topk(0, ids, True, 5)
    check(want_s, want_i, encodings(70, True), w.t, 5)
    bad = ids.copy()
    bad[33, -1] = V
    with pytest.raises(sse_amd.SSEError):
        h.encode_score_topk(0, bad, True, 5)
    again_s, again_i = h.encode_score_topk(0, ids, True, 5)
    assert np.array_equal(again_i, want_i) and np.array_equal(again_s, want_s)


def test_cluster_miss_at_q70_is_rerun_and_scored_again():
    """a cluster workgroup that does not arrive (option lstm_persist_inject_miss) sets the error flag the read-back brings home
    with an open certificate behind it: the batch is re-encoded on the kernels that need no co-residency and scored again"""
    w = world()
    h = w.m.handle
    ids = query_ids(w.pool, 70, True)
    paths = h.get_counter("lstm_path_cluster")
    want_s, want_i = h.encode_score_topk(0, ids, True, 5)
    assert h.get_counter("lstm_path_cluster") - paths == 1, "70 rows of this model do not take the cluster kernel"
    check(want_s, want_i, encodings(70, True), w.t, 5)
    falls = h.get_counter("lstm_persist_fallbacks")
    h.set_option("lstm_cluster_backoff", 0)                     # (the injected miss arms no back-off for the calls after it)
    h.set_option("lstm_persist_inject_miss", 1)
    try:
        got_s, got_i = h.encode_score_topk(0, ids, True, 5)
    finally:
        h.set_option("lstm_persist_inject_miss", 0)
        h.set_option("lstm_cluster_backoff", -1)                # (the default: automatic)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)
    assert h.get_counter("lstm_persist_fallbacks") - falls == 1
