"""Constructions shared by tests/test_gpu_score_rank.py (GPU) and tests/test_rank_metrics_host.py (CPU): index / query sets
whose float64 scores are EXACT in any summation order, so that the expected ranks do not depend on whose dot product formed
them.  The host test proves the exactness (two summation orders and fractions.Fraction); the GPU test relies on it."""
import numpy as np


def unit(rng, n, s):
    x = rng.standard_normal((n, s)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def ranks_from_scores(scores):
    """Inverse permutation of getSortedResults with the tie order 'lower row first': ranks[q, r] = position of row r."""
    order = np.argsort(-scores, axis=1, kind="stable")
    ranks = np.empty_like(order)
    np.put_along_axis(ranks, order, np.broadcast_to(np.arange(scores.shape[1]), order.shape), axis=1)
    return ranks


def quarter_set(seed, Q, N, S):
    """Entries k/4, k in -4 .. 4: every product is a multiple of 1/16 and every partial sum of <= 1024 of them is an
    integer multiple of 1/16 below 2^10 -- exact in float32 and float64, in any order (the construction of
    tests/test_gpu_score.py::test_exact_ties_rank_lower_row_first's sibling cases)."""
    rng = np.random.RandomState(seed)
    q = (rng.randint(-4, 5, size=(Q, S)) / 4.0).astype(np.float32)
    t = (rng.randint(-4, 5, size=(N, S)) / 4.0).astype(np.float32)
    return q, t


def exact_ties_case(seed=31, Q=5, N=300, S=32, copies=30):
    """Case 3: row N-1 is a copy of row 3; query 0 IS the row of largest norm (so that row and its copies are the strict
    maxima of query 0, Cauchy-Schwarz), and `copies` copies of it are scattered.  Returns (q, t, ids of the copies
    ascending, original included)."""
    q, t = quarter_set(seed, Q, N, S)
    n2 = (t.astype(np.float64) ** 2).sum(1)
    n2[[3, N - 1]] = -1.0
    b = int(np.argmax(n2))
    rng = np.random.RandomState(seed + 1)
    free = np.array([r for r in range(N) if r not in (3, N - 1, b)])
    spots = np.sort(rng.choice(free, size=copies, replace=False))
    t[spots] = t[b]
    t[N - 1] = t[3]
    q[0] = t[b]
    return q, t, np.sort(np.concatenate([spots, [b]]))


def near_tie_case(n_cluster, N, S=64, seed=41):
    """Cases 4 and 5: float64 index, queries e_0 and 2 e_0 (every other component zero: a score is ONE product, exact).
    Rows 0 .. n_cluster-1 scattered over the index are base + i 2^-30 e_0 with base[0] = 1/2: scores 1/2 + i 2^-30,
    strictly increasing in i, all within n_cluster 2^-30 of each other -- inside one fp32 band (2 (S + 2) 5.97e-8 = 7.9e-6
    at S = 64, times max|t| >= 1) while n_cluster <= 5000 (4.7e-6).  The other rows are random unit vectors.
    Returns (q float32 [2,S], t float64 [N,S], cluster row ids in order of i)."""
    rng = np.random.RandomState(seed)
    t = unit(rng, N, S).astype(np.float64)
    base = unit(rng, 1, S)[0].astype(np.float64)
    base[0] = 0.0
    base *= np.sqrt(0.75) / np.linalg.norm(base)
    base[0] = 0.5
    where = np.sort(rng.choice(N, size=n_cluster, replace=False))
    where = where[rng.permutation(n_cluster)]           # i does not ascend with the row id
    t[where] = base
    t[where, 0] = 0.5 + np.arange(n_cluster) * 2.0 ** -30
    q = np.zeros((2, S), np.float32)
    q[0, 0] = 1.0
    q[1, 0] = 2.0
    return q, t, where


def shard_case(seed=51, Q=17, N=4099, S=64):
    """Case 6: the quarter construction over N = 4099 rows, row 4000 a copy of row 10 (a tie across a cut at 2000)."""
    q, t = quarter_set(seed, Q, N, S)
    t[4000] = t[10]
    return q, t
