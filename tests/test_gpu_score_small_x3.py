"""The small-index scorer's split-bf16 candidate pass (option score_small_x3, default on; DESIGN K6): the candidates come
from qh.th + qh.tl + ql.th on the bf16 matrix pipe, every score that leaves the call is still the float64 re-scoring and
every id follows the float64 order.  So results are EQUAL -- to the fp32 candidates (option 0), to the list sweep
(score_small_index 0) and to the oracle -- or the bound handed to the certificate is wrong.

Shapes: the path needs >= 1024 queries; 1056 leaves a partial last 32-query tile.  Index rows 1 .. 1024 around the tile
(32), lane-register (640 / 641) and candidate-count (16) edges; dimensions of all three k-block classes with and without
zero padding (256 | 249, 64 | 57, 56 | 49)."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _unit(rng, n, s):
    x = rng.standard_normal((n, s)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _eps_x3(S, norm_max=1.0):
    """The documented candidate bound per unit query norm (DESIGN K6): truncation + accumulation with its factor 2."""
    return (2.0 ** -15 * (1 + 2.0 ** -6) + 2.0 * (3 * S + 2) * 2.0 ** -24 * (1 + 2.0 ** -5)) * norm_max


def _dev_topk(h, q, k):
    """sse_score_topk_dev: every stage queued (first stage, then lists_rest), no host check in between."""
    import torch
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
    out_s = torch.full((q.shape[0], k), float("nan"), dtype=torch.float64, device=dev)
    out_i = torch.full((q.shape[0], k), -7, dtype=torch.int64, device=dev)
    h.score_topk_dev(qd.data_ptr(), q.shape[0], k, out_s.data_ptr(), out_i.data_ptr())
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def _counters(h):
    return h.get_counter("score_collect_queries"), h.get_counter("score_bruteforce_queries")


def _oracle(q, t, k):
    return O.topk(O.scores_f64(q, np.asarray(t, np.float64)), k)


def _gap_10_16(q, t):
    """Smallest distance over the queries between the 10th and the 16th best exact score, per unit |q| max|t|."""
    s = -np.sort(-O.scores_f64(q, np.asarray(t, np.float64)), axis=1)
    scale = np.linalg.norm(q.astype(np.float64), axis=1) * np.linalg.norm(np.asarray(t, np.float64), axis=1).max()
    return float(((s[:, 9] - s[:, 15]) / scale).min())


def _score_tol(q, t, S):
    # float64 sums of S products in two different orders: <= 2 S 2^-53 |q||t| apart
    return 2.0 * S * 2.0 ** -53 * float(np.linalg.norm(q.astype(np.float64), axis=1).max() * np.linalg.norm(np.asarray(t, np.float64), axis=1).max())


@pytest.mark.parametrize("N,S", [(571, 256), (1024, 256), (641, 249), (571, 64), (571, 49), (1, 256), (15, 57), (16, 64),
                                 (17, 56), (33, 249), (640, 256), (641, 64), (1024, 49)])
def test_split_candidates_equal_fp32_candidates_and_the_list_sweep(N, S):
    """Option 1 against 0 and against the list sweep: np.array_equal on ids and float64 scores, host and device entry
    point; the oracle on the first and last 40 queries.  Exact ties (lower row first), 30 and 100 copies of a best row."""
    Q = 1056 if S in (256, 57, 49) else 1024
    rng = np.random.RandomState(N * 3 + S)
    q, t = _unit(rng, Q, S), _unit(rng, N, S)
    if N > 40:
        t[N - 1] = t[3]                                      # exact ties: the lower row first
        t[N // 2] = t[3]
        q[0] = t[3]
        for r in rng.choice(N, 30, replace=False):           # more exact copies than the 16 candidates hold
            t[r] = t[7]
        q[1] = t[7]
        q[Q - 2] = t[7]                                      # (also in the partial last tile)
    if N > 200:
        for r in rng.choice(N, 100, replace=False):          # more winners than the selection's 63 lanes
            t[r] = t[11]
        q[2] = t[11]
    q[Q - 1] *= 23.0
    h = _scorer()
    h.index_upload(t)
    k = min(10, N)
    sc, ids = h.score_topk(q, k)
    dsc, dids = _dev_topk(h, q, k)
    assert np.array_equal(ids, dids) and np.array_equal(sc, dsc)
    h.set_option("score_small_x3", 0)
    sc32, ids32 = h.score_topk(q, k)
    assert np.array_equal(ids, ids32) and np.array_equal(sc, sc32)
    h.set_option("score_small_x3", 1)
    h.set_option("score_small_index", 0)
    sc0, ids0 = h.score_topk(q, k)
    assert np.array_equal(ids, ids0) and np.array_equal(sc, sc0)
    sub = np.concatenate([np.arange(40), np.arange(Q - 40, Q)])
    wsc, wids = _oracle(q[sub], t, k)
    assert np.array_equal(ids[sub], wids)
    assert np.abs(sc[sub] - wsc).max() <= _score_tol(q, t, S)


def _crowded(rng, Q, N, S, step, crowded_queries=(0,)):
    """Query 0 (and copies of it) with 40 index rows c * base + sqrt(1 - c^2) * u, c = 1 - step * j: exact scores `step` apart."""
    t = _unit(rng, N, S).astype(np.float64)
    q = _unit(rng, Q, S)
    for c in crowded_queries:
        q[c] = q[0]
    base = q[0].astype(np.float64)
    base /= np.linalg.norm(base)
    for j, r in enumerate(rng.choice(N, 40, replace=False)):
        u = rng.standard_normal(S)
        u -= u.dot(base) * base
        u /= np.linalg.norm(u)
        c = 1.0 - step * j
        t[r] = c * base + np.sqrt(1.0 - c * c) * u
    return q, t


@pytest.mark.parametrize("S", [256, 64])
def test_scores_packed_tighter_than_the_bound_take_the_collect_pass(S):
    """40 rows whose exact scores sit 2e-6 apart: below any valid candidate bound, and more than 16 of them within it.  The
    certificate must fail, the collect pass serves the query, results equal the oracle's."""
    rng = np.random.RandomState(5 + S)
    Q, N = 1024, 571
    q, t = _crowded(rng, Q, N, S, 2e-6)
    h = _scorer()
    h.index_upload(t)
    c0, b0 = _counters(h)
    sc, ids = h.score_topk(q, 10)
    c1, b1 = _counters(h)
    wsc, wids = _oracle(q, t, 10)
    assert np.array_equal(ids, wids) and np.abs(sc - wsc).max() <= max(1e-12, _score_tol(q, t, S))
    assert c1 - c0 >= 1 and b1 == b0
    dsc, dids = _dev_topk(h, q, 10)
    assert np.array_equal(ids, dids) and np.array_equal(sc, dsc)


@pytest.mark.parametrize("S", [256, 64])
def test_scores_a_thousandth_apart_keep_their_certificate(S):
    rng = np.random.RandomState(9 + S)
    Q, N = 1024, 571
    q, t = _crowded(rng, Q, N, S, 1e-3)
    assert _gap_10_16(q, t) > 3 * _eps_x3(S)                 # the data: no query within reach of the bound
    h = _scorer()
    h.index_upload(t)
    before = _counters(h)
    sc, ids = h.score_topk(q, 10)
    wsc, wids = _oracle(q, t, 10)
    assert np.array_equal(ids, wids) and np.abs(sc - wsc).max() <= max(1e-12, _score_tol(q, t, S))
    assert _counters(h) == before


def test_certified_and_uncertified_queries_share_query_blocks_on_the_device_entry_point():
    """Q = 1056, crowded queries in the first, a middle and the partial last 32-query tile, all stages queued at once."""
    rng = np.random.RandomState(77)
    Q, N, S = 1056, 571, 256
    q, t = _crowded(rng, Q, N, S, 2e-6, crowded_queries=(0, 5, 517, 1055))
    h = _scorer()
    h.index_upload(t)
    c0, b0 = _counters(h)
    dsc, dids = _dev_topk(h, q, 10)
    c1, b1 = _counters(h)
    wsc, wids = _oracle(q, t, 10)
    assert np.array_equal(dids, wids) and np.abs(dsc - wsc).max() <= max(1e-12, _score_tol(q, t, S))
    assert c1 - c0 >= 4 and b1 == b0
    sc, ids = h.score_topk(q, 10)
    assert np.array_equal(ids, dids) and np.array_equal(sc, dsc)


@pytest.mark.parametrize("N,S", [(571, 256), (571, 64)])
def test_benign_data_never_leaves_the_certified_path(N, S):
    """Random unit vectors: the wider bound must not send a single query to the collect pass or the float64 sweep --
    otherwise the speed is not real."""
    rng = np.random.RandomState(N + S)
    q, t = _unit(rng, 1024, S), _unit(rng, N, S)
    assert _gap_10_16(q, t) > 3 * _eps_x3(S)
    h = _scorer()
    h.index_upload(t)
    before = _counters(h)
    sc, ids = h.score_topk(q, 10)
    assert _counters(h) == before
    wsc, wids = _oracle(q, t, 10)
    assert np.array_equal(ids, wids) and np.abs(sc - wsc).max() <= max(1e-12, _score_tol(q, t, S))


@pytest.mark.parametrize("S", [256, 57])
def test_magnitudes_of_queries_and_index_rows(S):
    """Queries scaled by 23 and by 1e-3 (the bound scales with |q| inside the kernel), index rows of norm 0.02 .. 50 in one
    index (the bound scales with the largest row norm): exact against the oracle."""
    rng = np.random.RandomState(31 + S)
    Q, N = 1056, 571
    q, t = _unit(rng, Q, S), _unit(rng, N, S)
    q[0::3] *= np.float32(23.0)
    q[1::3] *= np.float32(1e-3)
    t *= np.exp(rng.uniform(np.log(0.02), np.log(50.0), size=(N, 1))).astype(np.float32)
    h = _scorer()
    h.index_upload(t)
    sc, ids = h.score_topk(q, 10)
    wsc, wids = _oracle(q, t, 10)
    assert np.array_equal(ids, wids)
    qn = np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    assert (np.abs(sc - wsc) / qn).max() <= 2.0 * S * 2.0 ** -53 * float(np.linalg.norm(t.astype(np.float64), axis=1).max())
    h.set_option("score_small_x3", 0)
    sc32, ids32 = h.score_topk(q, 10)
    assert np.array_equal(ids, ids32) and np.array_equal(sc, sc32)


@pytest.mark.parametrize("entry", ["index_upload", "index_set_dev"])
def test_no_stale_split_image_after_an_index_change(entry):
    """One handle: 571 rows, then a different index of 300 rows, then the first again (and one of another dimension in
    between); every result equals a fresh handle's and nothing leaves the certified path."""
    import torch
    rng = np.random.RandomState(3)
    Q = 1024
    idx = [_unit(rng, 571, 256), _unit(rng, 300, 256), _unit(rng, 571, 64)]
    qs = {256: _unit(rng, Q, 256), 64: _unit(rng, Q, 64)}
    keep = []

    def set_index(h, t):
        if entry == "index_upload":
            h.index_upload(t)
        else:
            d = torch.from_numpy(t).to("cuda:0")
            keep.append(d)
            h.index_set_dev(d.data_ptr(), t.shape[0], t.shape[1])
            torch.cuda.synchronize()

    def fresh(t):
        h = _scorer()
        set_index(h, t)
        return h.score_topk(qs[t.shape[1]], 10)

    assert all(_gap_10_16(qs[t.shape[1]], t) > 3 * _eps_x3(t.shape[1]) for t in idx)
    want = [fresh(t) for t in idx]
    h = _scorer()
    before = _counters(h)
    for i in (0, 1, 0, 2, 1, 0):
        set_index(h, idx[i])
        sc, ids = h.score_topk(qs[idx[i].shape[1]], 10)
        assert np.array_equal(ids, want[i][1]) and np.array_equal(sc, want[i][0]), i
    assert _counters(h) == before
    wsc, wids = _oracle(qs[256], idx[0], 10)
    assert np.array_equal(want[0][1], wids)


def test_follow_up_launches_over_consecutive_calls():
    """The re-scoring pass counts its uncertified queries in a device word that the follow-up launches read first; two
    words are used in turn and each call clears the next call's.  Calls with and without uncertified queries in every
    order on one handle, both entry points: the collect pass must serve the crowded queries each time."""
    rng = np.random.RandomState(123)
    Q, N, S = 1056, 571, 256
    qc, t = _crowded(rng, Q, N, S, 2e-6, crowded_queries=(0, 1055))
    # the same batch without the crowded queries: they, and every query the 40 packed rows come near the bound for, are
    # replaced by copies of a query that is far from it
    s = -np.sort(-O.scores_f64(qc, t), axis=1)
    near = (s[:, 9] - s[:, 15]) <= 5 * _eps_x3(S)
    assert near[0] and near[1055] and near.sum() < Q // 4
    qb = qc.copy()
    qb[near] = qc[np.flatnonzero(~near)[0]]
    assert _gap_10_16(qb, t) > 3 * _eps_x3(S)
    want = {"c": _oracle(qc, t, 10), "b": _oracle(qb, t, 10)}
    h = _scorer()
    h.index_upload(t)
    tol = max(1e-12, _score_tol(qc, t, S))
    for n, which in enumerate("cbbccbcb"):
        q = qc if which == "c" else qb
        c0, b0 = _counters(h)
        sc, ids = _dev_topk(h, q, 10) if n % 3 else h.score_topk(q, 10)
        c1, b1 = _counters(h)
        assert np.array_equal(ids, want[which][1]) and np.abs(sc - want[which][0]).max() <= tol, (n, which)
        assert (c1 - c0 >= 2 if which == "c" else c1 == c0) and b1 == b0, (n, which, c1 - c0)
