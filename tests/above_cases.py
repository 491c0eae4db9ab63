"""Constructions and the float64 reference shared by tests/test_gpu_score_above.py (GPU), tests/above_two_rank_worker.py and
tests/test_above_cases_host.py (CPU).  Like tests/rank_cases.py (imported, not edited): index / query sets whose float64 scores
are EXACT in any summation order, so that the expected segments do not depend on whose dot product formed them.  The host test
proves the exactness; the GPU tests rely on it."""
import numpy as np

SORT_CAP = 8192          # SSE_ABOVE_SORT_CAP (csrc/sse_kernels.h): entries one workgroup sorts in LDS; longer segments are merged
LADDER_N = 20011


def expected_above(scores, pair_q, thr, id_base=0):
    """scores float64 [Q, N] -> (offsets int64 [L+1], ids int64 [total], scores float64 [total]): for pair p the rows r with
    scores[pair_q[p], r] >= thr[p] (IEEE: NaN and +inf match nothing), score descending, equal scores by ascending id."""
    scores = np.asarray(scores, np.float64)
    pair_q, thr = np.asarray(pair_q, np.int64).reshape(-1), np.asarray(thr, np.float64).reshape(-1)
    offsets = np.zeros(len(thr) + 1, np.int64)
    ids, out = [], []
    order_of = {}
    for p in range(len(thr)):
        qi = int(pair_q[p])
        if qi not in order_of:
            order_of[qi] = np.argsort(-scores[qi], kind="stable")       # descending, lower row first among equals
        order = order_of[qi]
        with np.errstate(invalid="ignore"):
            keep = order[scores[qi, order] >= thr[p]]
        offsets[p + 1] = offsets[p] + len(keep)
        ids.append(keep.astype(np.int64) + id_base)
        out.append(scores[qi, keep])
    if not ids:
        return offsets, np.zeros(0, np.int64), np.zeros(0, np.float64)
    return offsets, np.concatenate(ids), np.concatenate(out)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def assert_above_equal(got, want, exact_scores=True):
    """offsets equal, ids equal, scores the same 64 bits (exact_scores=False: within the project's 1e-12)."""
    go, gi, gs = (np.asarray(x) for x in got)
    wo, wi, ws = (np.asarray(x) for x in want)
    assert go.shape == wo.shape and np.array_equal(go, wo), "offsets differ"
    assert gi.shape == wi.shape and np.array_equal(gi, wi), "ids differ"
    assert gs.shape == ws.shape
    if exact_scores:
        assert np.array_equal(bits(gs), bits(ws)), "score bits differ"
    elif len(ws):
        assert np.abs(gs - ws).max() < 1e-12, "scores differ"


def ladder_perm(N=LADDER_N, seed=71):
    return np.random.RandomState(seed).permutation(N)


def ladder_case(N=LADDER_N, S=64, seed=71):
    """Row r = (pi(r) + 1) 2^-15 e_0 for a fixed permutation pi, query e_0: score (pi(r) + 1) 2^-15 -- ONE product of a power
    of two and an integer below 2^15, exact in float32 and float64 -- strictly increasing in pi(r) and 2^-15 = 3.05e-5 apart,
    wider than the fp32 band 2 (S + 2) 5.97e-8 max|t| < 7.9e-6: any count can be dialled, no row sits in a band but the one AT
    the threshold.  Returns (q float32 [1,S], t float32 [N,S], pi)."""
    assert N <= 32768
    pi = ladder_perm(N, seed)
    t = np.zeros((N, S), np.float32)
    t[:, 0] = ((pi + 1) * 2.0 ** -15).astype(np.float32)
    q = np.zeros((1, S), np.float32)
    q[0, 0] = 1.0
    return q, t, pi


def ladder_threshold(count, N=LADDER_N):
    """the threshold that exactly `count` rows of the ladder reach (count in [0, N])"""
    return (N - count + 1) * 2.0 ** -15


def ladder_counts(N=LADDER_N):
    """2^k - 1, 2^k, 2^k + 1 for k = 0 .. 14, and N; SORT_CAP = 2^13 is among them with both neighbours."""
    c = sorted({v for k in range(15) for v in (2 ** k - 1, 2 ** k, 2 ** k + 1) if v <= N} | {N, SORT_CAP - 1, SORT_CAP, SORT_CAP + 1})
    return np.array(c, np.int64)


def near_duplicate_rows(seed=81, N=300, S=32, copies=12, near=5):
    """300 unit rows with 12 planted exact copies and 5 planted near-copies (a copy with one component nudged and
    re-normalised: cosine ~ 1 - 1e-4).  Returns t float32 [N,S]."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((N, S)).astype(np.float32)
    t = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    spots = rng.choice(N, size=2 * (copies + near), replace=False)
    src, dst = spots[:copies + near], spots[copies + near:]
    for i in range(copies):
        t[dst[i]] = t[src[i]]
    for i in range(copies, copies + near):
        v = t[src[i]].astype(np.float64)
        v[i % S] += 0.015
        t[dst[i]] = (v / np.linalg.norm(v)).astype(np.float32)
    return t


def expected_near_duplicates(scores, threshold):
    """pairs (i, j, score) with i < j and scores[i, j] >= threshold, sorted by (i, j)"""
    i, j = np.nonzero(np.triu(scores >= threshold, k=1))
    return [(int(a), int(b), float(scores[a, b])) for a, b in zip(i, j)]
