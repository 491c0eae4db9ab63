"""rescore_small4_kernel (four queries per re-score wave, DESIGN K6) against rescore_small_kernel, which the environment
variable SSE_RESCORE_SMALL4=0 puts back (read at every launch): the same handle and inputs through both, and everything the
call hands back has to be IDENTICAL -- float64 scores as bit patterns, ids, and what the certificates sent to the collect
pass and to the float64 sweep (counter deltas).  Ids and scores against the float64 oracle as well.

Shapes: the small-index route needs >= 1024 queries; 1025 and 1027 leave one and three rows of the last wave's four (and
fifteen and thirteen rows of the last workgroup's sixteen) past the end.  Index rows: 5 with k = 3 (empty candidate slots),
16 (every slot a candidate), 17, 571; dimensions of the three k-block classes (256; 64; 50: a partial last group of four and
virtual lanes without dimensions); k = 1, 10, 16.

The same change lets the split-bf16 scorer stage a workgroup's query rows through LDS once instead of loading them in every
wave: Q = 1041 (a last tile of 17 queries) at S = 256 and 64 against the fp32 scorer, the list sweep and the oracle."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

ENV = "SSE_RESCORE_SMALL4"


@pytest.fixture(scope="module")
def handle():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


@pytest.fixture(autouse=True)
def _env_restored():
    old = os.environ.get(ENV)
    yield
    if old is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = old


def _unit(rng, n, s):
    x = rng.standard_normal((n, s)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _dev_topk(h, q, k):
    import torch
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
    out_s = torch.full((q.shape[0], k), float("nan"), dtype=torch.float64, device=dev)
    out_i = torch.full((q.shape[0], k), -7, dtype=torch.int64, device=dev)
    h.score_topk_dev(qd.data_ptr(), q.shape[0], k, out_s.data_ptr(), out_i.data_ptr())
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def _counters(h):
    return np.array([h.get_counter("score_collect_queries"), h.get_counter("score_bruteforce_queries")])


def _both_arms(h, q, k, call=_dev_topk):
    """(scores, ids, counter deltas) of the one-query-per-wave kernel and of the four-queries one; asserts them identical."""
    out = []
    for arm in ("0", None):
        if arm is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = arm
        c0 = _counters(h)
        sc, ids = call(h, q, k)
        out.append((sc, ids, _counters(h) - c0))
    (sc0, ids0, d0), (sc4, ids4, d4) = out
    assert np.array_equal(ids0, ids4)
    assert np.array_equal(np.ascontiguousarray(sc0).view(np.int64), np.ascontiguousarray(sc4).view(np.int64))
    assert np.array_equal(d0, d4), (d0, d4)
    return sc4, ids4, d4


def _score_tol(q, t, S):
    # float64 sums of S products in two different orders: <= 2 S 2^-53 |q||t| apart
    return 2.0 * S * 2.0 ** -53 * float(np.linalg.norm(q.astype(np.float64), axis=1).max() * np.linalg.norm(np.asarray(t, np.float64), axis=1).max())


def _check_oracle(q, t, k, sc, ids):
    wsc, wids = O.topk(O.scores_f64(q, np.asarray(t, np.float64)), k)
    assert np.array_equal(ids, wids)
    assert np.abs(sc - wsc).max() <= max(1e-12, _score_tol(q, t, q.shape[1]))


@pytest.mark.parametrize("S", [256, 64, 50])
@pytest.mark.parametrize("N", [5, 16, 17, 571])
def test_identical_to_the_one_query_wave_and_equal_to_the_oracle(handle, N, S):
    rng = np.random.RandomState(N * 5 + S)
    t = _unit(rng, N, S)
    handle.index_upload(t)
    for Q, k in ((1024, 10), (1025, 1), (1027, 16)):
        k = 3 if N == 5 else min(k, N)
        q = _unit(rng, Q, S)
        q[Q - 1] *= np.float32(23.0)
        q[Q // 2] *= np.float32(1e-3)
        sc, ids, _ = _both_arms(handle, q, k)
        _check_oracle(q, t, k, sc, ids)


@pytest.mark.parametrize("S", [256, 50])
def test_host_entry_point(handle, S):
    rng = np.random.RandomState(S)
    Q, N = 1027, 571
    q, t = _unit(rng, Q, S), _unit(rng, N, S)
    handle.index_upload(t)
    sc, ids, _ = _both_arms(handle, q, 10, call=lambda h, q, k: h.score_topk(q, k))
    _check_oracle(q, t, 10, sc, ids)
    dsc, dids = _dev_topk(handle, q, 10)
    assert np.array_equal(ids, dids) and np.array_equal(sc, dsc)


@pytest.mark.parametrize("S,k", [(256, 10), (64, 16), (50, 1)])
def test_duplicated_index_rows_rank_by_lower_id(handle, S, k):
    """Exact copies of a best row inside the candidates (3 and 12 of them) and more copies than the 16 candidates hold (30):
    equal float64 scores, the lower row first."""
    rng = np.random.RandomState(11 + S)
    Q, N = 1025, 571
    q, t = _unit(rng, Q, S), _unit(rng, N, S)
    t[N - 1] = t[3]
    t[N // 2] = t[3]
    for r in rng.choice(np.arange(20, N - 1), 11, replace=False):
        t[r] = t[5]
    for r in rng.choice(np.arange(20, N - 1), 30, replace=False):
        t[r] = t[7]
    q[0] = t[3]
    q[1] = t[5]
    q[Q - 1] = t[5]
    q[2] = t[7]
    q[Q - 2] = t[7]
    handle.index_upload(t)
    sc, ids, _ = _both_arms(handle, q, k)
    # The oracle's matrix product may sum two equal rows in different orders, so its order among copies says nothing.
    # What holds: the score lists agree, every id carries its own score, equal scores come lower id first, and a query that
    # IS a copied row gets that row's copies, lowest ids first, in front of everything else (copies score 1, the rest less).
    want = O.scores_f64(q, np.asarray(t, np.float64))
    tol = max(1e-12, _score_tol(q, t, S))
    assert np.abs(sc - (-np.sort(-want, axis=1))[:, :k]).max() <= tol
    assert np.abs(sc - np.take_along_axis(want, ids, axis=1)).max() <= tol
    assert all(len(set(r)) == k for r in ids)
    tied = sc[:, :-1] == sc[:, 1:]
    assert (sc[:, :-1] >= sc[:, 1:]).all() and (ids[:, :-1] < ids[:, 1:])[tied].all()
    for qi, x in ((0, 3), (1, 5), (Q - 1, 5), (2, 7), (Q - 2, 7)):
        group = np.flatnonzero((t == t[x]).all(axis=1))
        m = min(k, len(group))
        assert np.array_equal(ids[qi, :m], group[:m]), (qi, x)


@pytest.mark.parametrize("S", [256, 64])
def test_a_crowded_query_fails_its_certificate_and_the_tail_serves_it(handle, S):
    """40 rows whose exact scores sit 2e-6 apart around one query (and around its copies in the last, partial wave): more
    than 16 within the candidate bound, so the certificate fails in both kernels alike and the collect pass answers."""
    rng = np.random.RandomState(5 + S)
    Q, N = 1027, 571
    t = _unit(rng, N, S).astype(np.float64)
    q = _unit(rng, Q, S)
    q[517] = q[0]
    q[Q - 1] = q[0]
    base = q[0].astype(np.float64)
    base /= np.linalg.norm(base)
    for j, r in enumerate(rng.choice(N, 40, replace=False)):
        u = rng.standard_normal(S)
        u -= u.dot(base) * base
        u /= np.linalg.norm(u)
        c = 1.0 - 2e-6 * j
        t[r] = c * base + np.sqrt(1.0 - c * c) * u
    handle.index_upload(t)
    sc, ids, delta = _both_arms(handle, q, 10)
    assert delta[0] >= 3 and delta[1] == 0
    _check_oracle(q, t, 10, sc, ids)


@pytest.mark.parametrize("S", [256, 50])
def test_float64_index_rows(handle, S):
    """An index uploaded as float64 is re-scored from its float64 rows (a lane's dimensions are v, v + 64, ... there)."""
    rng = np.random.RandomState(41 + S)
    Q, N = 1027, 571
    q = _unit(rng, Q, S)
    t = rng.standard_normal((N, S))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    handle.index_upload(t)
    sc, ids, _ = _both_arms(handle, q, 10)
    _check_oracle(q, t, 10, sc, ids)


@pytest.mark.parametrize("S", [256, 64])
@pytest.mark.parametrize("N", [571, 20])
def test_scorer_query_tile_staged_through_lds(handle, N, S):
    """The split-bf16 scorer stages a workgroup's 32 query rows through the score tile's LDS when whole rows fit in it (571
    rows: yes; 20 rows: the tile is too small, direct loads).  Q = 1041 ends in a tile of 17 queries: one wave stages a
    single real row, one none.  Results equal the fp32 scorer's (option score_small_x3 = 0, which does not stage), the list
    sweep's and the oracle's."""
    rng = np.random.RandomState(N + S)
    Q = 1041
    q, t = _unit(rng, Q, S), _unit(rng, N, S)
    q[Q - 1] *= np.float32(23.0)
    q[1024] *= np.float32(1e-3)
    handle.index_upload(t)
    sc, ids, _ = _both_arms(handle, q, 10)
    _check_oracle(q, t, 10, sc, ids)
    try:
        handle.set_option("score_small_x3", 0)
        sc32, ids32 = _dev_topk(handle, q, 10)
        assert np.array_equal(ids, ids32) and np.array_equal(sc, sc32)
    finally:
        handle.set_option("score_small_x3", 1)
    try:
        handle.set_option("score_small_index", 0)
        sc0, ids0 = _dev_topk(handle, q, 10)
        assert np.array_equal(ids, ids0) and np.array_equal(sc, sc0)
    finally:
        handle.set_option("score_small_index", 1)


@pytest.mark.parametrize("S", [256, 50])
def test_all_zero_query_rows(handle, S):
    """|q| = 0: every score is 0.0, the error bound is 0, and the order is the row id's; zero rows in the first wave, in
    a row of their own between others, and in the partial last wave."""
    rng = np.random.RandomState(21 + S)
    Q, N = 1025, 571
    q, t = _unit(rng, Q, S), _unit(rng, N, S)
    for r in (0, 1, 6, 515, Q - 1):
        q[r] = 0.0
    handle.index_upload(t)
    sc, ids, _ = _both_arms(handle, q, 10)
    _check_oracle(q, t, 10, sc, ids)
    assert np.array_equal(ids[0], np.arange(10)) and not sc[0].any()
