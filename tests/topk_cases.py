"""Cases shared by tests/test_gpu_score_large_k.py (GPU) and tests/test_topk_cases_host.py (CPU): top-k above 16 on both of its
routes -- the select route (17 <= k <= 1024: candidate sweep, threshold from the k-th candidate, collect sweep, float64 sort)
and exact paging in pages of 16 (k > 1024, and every query whose collect buffer overflowed) -- and two k <= 16 neighbours of
the paging code (the strided brute force with open queries, the collect-slot pool running out).  DESIGN K6.

One list, CASES.  Per case: inputs(case) builds (q, t) from the case's seed, expected(case) is the float64 reference with
id_base added, preconditions(case) proves the reference is one the device can be held to (ties are exact ties, everything
else is further apart than two float64 summation orders can move it), check(case, scores, ids) is what both entry points'
results must pass.  The counter deltas a call must cause are part of the case; they are derived from the code:

  select route    select_topk_query adds 1 to score_collect_queries per query it serves; a query it leaves (more than
                  SSE_COLLECT_CAP = 4096 rows at or above the threshold) goes to exact_topk_query, which adds 1 to
                  score_bruteforce_queries on the first page only
  k > 1024        launch_exact_topk is given no counter: both stay
  k <= 16         an uncertified query takes a collect slot (1024 per call, TopkPlan::POOL set by topk_plan) and is served by the
                  select kernel unless its buffer overflows; without a slot, or after an overflow: brute force

No GPU import here."""
import functools

import numpy as np

from oracle import sse_oracle as O

BASE = 1_000_000_007      # a shard's first global row id: not a multiple of anything, above 2^29
COLLECT_CAP = 4096        # SSE_COLLECT_CAP
SLOT_POOL = 1024          # TopkPlan::POOL (topk_plan in csrc/sse_api.hip)


class Case:
    def __init__(self, name, Q, N, S, k, kind="benign", id_base=0, upload="f32", options=(), seed=0, collect=None, brute=0,
                 copies=0, planted=(), zero=(), ordinary_below=False, why=""):
        self.name, self.Q, self.N, self.S, self.k = name, Q, N, S, k
        self.kind = kind              # benign | tie | zero | dup | all_equal
        self.id_base = id_base
        self.upload = upload          # f32: index_upload(float32) | f64: index_upload(float64) | dev: index_set_dev
        self.options = options        # ((name, (values ...)), ...): the call is repeated per value, results np.array_equal
        self.seed = seed
        self.collect = Q if collect is None else collect   # delta of score_collect_queries per call; -1: not derived
        self.brute = brute                                 # delta of score_bruteforce_queries per call
        self.copies = copies          # rows that are bit-equal copies of one row (the original included)
        self.planted = tuple(planted)  # queries equal to that row
        self.zero = tuple(zero)       # all-zero queries
        self.ordinary_below = ordinary_below  # the other queries score the copied row below zero (see inputs)
        self.why = why

    def __repr__(self):
        return self.name


def _benign(name, Q, N, S, k, **kw):
    return Case(name, Q, N, S, k, seed=kw.pop("seed", 1000 + Q + N + S + k), **kw)


def strided_case(Q=600):
    """exact_topk_strided_kernel is launched when Q exceeds the follow-up grid, 2 * cu_count = 512 on the 256 CUs of an MI355X:
    Q = 600.  (A device with more than 300 CUs: the GPU test asks for Q past twice its count; the planted queries move along --
    the first, the last of the first half, one in a late workgroup's second round, the last.)  4500 copies overflow the
    collect buffer of the four queries that are the copied row: brute = 4.  The others score the copies below zero: whether
    certified or collected they stay away from the brute force; how many of them the collect pass serves is not derived."""
    return Case("strided_open_q%d" % Q, Q, 6000, 64, 10, kind="dup", seed=77, copies=4500, planted=(0, Q // 2 - 1, Q - 89, Q - 1),
                ordinary_below=True, collect=-1, brute=4, why="k <= 16: strided brute force with open queries")


CASES = [
    # ---- benign: random unit rows, every query served by the select route (collect = Q, brute = 0) unless noted
    _benign("fewer_candidates_than_k", 1, 100, 16, 90, why="threshold -inf, every row collected, 4 padding rows stay out"),
    _benign("k_is_n_tail_tile_of_one", 2, 33, 5, 33, why="k = N, one row in the tail tile, S < 8"),
    _benign("k17", 5, 3000, 32, 17, why="smallest k of the route"),
    _benign("q33_nq4_partial_tile", 33, 2000, 64, 64, why="Q > 32: NQ = 4, partial second query tile"),
    _benign("s300_nq2_unringed", 40, 700, 300, 40, why="S > 296: NQ = 2, KG = 38 not a multiple of 8"),
    _benign("s620_nq1_q40", 40, 700, 620, 40, why="S > 616: NQ = 1 with Q > 32"),
    _benign("k1024", 3, 1100, 64, 1024, why="k = SSE_MAX_SELECT_K"),
    _benign("k1025_paging", 3, 1100, 64, 1025, collect=0, why="first k of pure paging, 65 pages, no counter passed"),
    _benign("k_is_n_paging", 3, 1100, 64, 1100, collect=0, why="k = N by paging"),
    _benign("second_pool", 2080, 300, 16, 20, why="Q > 2048: second pool of 32 queries"),
    _benign("n9000_bf16_on_off", 129, 9000, 64, 100, options=(("score_bf16", (1, 0)),), why="N >= 8192: option has no say for k > 16"),
    _benign("f64_rows", 20, 1500, 48, 30, upload="f64", seed=4242, why="float64 index: idx64 branch of wave_exact_dot"),
    _benign("f64_rows_rounded", 20, 1500, 48, 30, upload="f32", seed=4242, why="the same rows rounded to float32"),
    _benign("dev_index_id_base", 9, 1200, 40, 33, upload="dev", id_base=BASE, why="index_set_dev with a shard base"),
    # ---- ties and overflows
    Case("tie_across_kth", 9, 2000, 32, 20, kind="tie", seed=11, copies=30, planted=(4,),
         why="30 copies, k = 20: first tile, every split, last partial tile"),
    Case("zero_query_n3000", 5, 3000, 32, 40, kind="zero", seed=12, zero=(2,), why="3000 equal keys sorted by row"),
    Case("zero_query_n5000", 5, 5000, 32, 40, kind="zero", seed=13, zero=(2,), collect=4, brute=1,
         why="5000 > 4096: overflow into paging, both cuts inside the tie run"),
    Case("zero_query_n5000_base", 5, 5000, 32, 40, kind="zero", seed=13, zero=(2,), collect=4, brute=1, id_base=BASE,
         why="the same with a shard base: the cut subtracts it"),
    Case("dup_overflow", 8, 6000, 64, 50, kind="dup", seed=14, copies=4500, planted=(3,), ordinary_below=True, collect=7, brute=1,
         why="4500 copies > 4096: paging inside the copies"),
    Case("dup_overflow_base", 8, 6000, 64, 50, kind="dup", seed=14, copies=4500, planted=(3,), ordinary_below=True, collect=7,
         brute=1, id_base=BASE, why="the same with a shard base"),
    # ---- k <= 16 neighbours of the same fallback code (fp32 candidates: N < 8192)
    strided_case(600),
    Case("slot_pool_exhausted", 1100, 6000, 64, 10, kind="all_equal", seed=78, copies=600, planted=tuple(range(1100)),
         collect=SLOT_POOL, brute=1100 - SLOT_POOL, why="k <= 16: 1100 uncertified queries, 1024 slots"),
]
BY_NAME = {c.name: c for c in CASES}


def unit(rng, n, s, dtype=np.float32):
    x = rng.standard_normal((n, s))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(dtype)


def _copy_rows(case):
    """Where the copies sit: the first tile, the last (partial) tile, the rest evenly over the index -- every split of the sweep
    sees some.  Ascending; the first is the original."""
    N, c = case.N, case.copies
    if c >= N // 2:                                       # crowds: every fourth row stays ordinary
        rows = np.array([r for r in range(N) if r % 4 != 1][:c])
    else:
        rows = np.unique(np.concatenate([[3, 17, N - 10, N - 1], np.linspace(40, N - 40, c - 4).astype(np.int64)]))
    assert rows.size == c, (rows.size, c)
    return rows


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(q float32 [Q,S], t float32 or float64 [N,S], rows of the copy group ascending (or empty)); read-only."""
    rng = np.random.RandomState(case.seed)
    # (unit() normalises in float64 and rounds last: f64_rows_rounded, same seed, IS f64_rows rounded to float32)
    t = unit(rng, case.N, case.S, np.float64 if case.upload == "f64" else np.float32)
    group = np.zeros(0, np.int64)
    if case.kind == "all_equal":
        q = np.empty((case.Q, case.S), np.float32)
    else:
        q = unit(rng, case.Q, case.S)
    if case.copies:
        group = _copy_rows(case)
        t[group] = t[group[0]]
        if case.ordinary_below:
            # the other queries must not see the 4500 copies anywhere near their top-k (their counters are derived on that): a
            # query that scores the copied row above zero is negated -- still a random unit vector for every other row
            flip = q.astype(np.float64) @ t[group[0]].astype(np.float64) > 0
            q[flip] = -q[flip]
        q[list(case.planted)] = t[group[0]]
    for z in case.zero:
        q[z] = 0.0
    for a in (q, t, group):
        a.setflags(write=False)
    return q, t, group


def scales(case):
    """(|q| max, |t| max, tol): tol bounds the distance of two float64 sums of S products in different orders
    (tests/test_gpu_score_small_x3.py::_score_tol)."""
    q, t, _ = inputs(case)
    qn = float(np.linalg.norm(q.astype(np.float64), axis=1).max())
    tn = float(np.linalg.norm(np.asarray(t, np.float64), axis=1).max())
    return qn, tn, 2.0 * case.S * 2.0 ** -53 * qn * tn


def score_bar(case):
    qn, tn, tol = scales(case)
    return max(1e-12 * qn * tn, tol)


@functools.lru_cache(maxsize=None)
def reference_scores(case):
    """O.scores_f64 of the case, [Q, N], read-only.  A case with planted copies takes the product against the index with the
    copies left out and hands every copy the column of the original: bit-equal rows have ONE reference score.  (The BLAS
    behind np.dot may form the columns of a matrix edge in another order than the body's -- equal here today, nothing a test
    should stand on.)  A case whose queries are all the same row forms one row of scores."""
    q, t, group = inputs(case)
    t64 = np.asarray(t, np.float64)
    qq = q[:1] if case.kind == "all_equal" else q
    if group.size:
        keep = np.ones(case.N, bool)
        keep[group[1:]] = False
        col = np.cumsum(keep) - 1                            # column of the reduced product per row ...
        col[group] = col[group[0]]                           # ... and the original's for every copy
        s = O.scores_f64(qq, t64[keep])[:, col]
    else:
        s = O.scores_f64(qq, t64)
    if case.kind == "all_equal":
        s = np.broadcast_to(s, (case.Q, case.N))
    s = np.ascontiguousarray(s)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def reference(case, k=None):
    """(scores float64 [Q,k], ids int64 [Q,k] + id_base) in getSortedResults' order, ties by lower row; read-only."""
    k = case.k if k is None else k
    s = reference_scores(case)
    if case.kind == "all_equal":
        ws, wi = O.topk(s[:1], k)
        ws, wi = np.repeat(ws, case.Q, 0), np.repeat(wi, case.Q, 0)
    else:
        ws, wi = O.topk(s, k)                                # (a stable sort of all N columns: no slack to run out of in a tie)
    ws, wi = np.ascontiguousarray(ws), np.ascontiguousarray(wi.astype(np.int64) + case.id_base)
    ws.setflags(write=False)
    wi.setflags(write=False)
    return ws, wi


def expected(case):
    return reference(case)


def preconditions(case):
    """AssertionError unless the reference is one a device summing in its own order must reproduce id for id."""
    q, t, group = inputs(case)
    s = reference_scores(case)
    qn, tn, tol = scales(case)
    assert q.shape == (case.Q, case.S) and t.shape == (case.N, case.S) and 1 <= case.k <= case.N
    in_group = np.zeros(case.N, bool)
    if group.size:
        assert group.size == case.copies and (np.diff(group) > 0).all()
        tb = np.ascontiguousarray(t[group])
        assert (tb.view(np.uint8) == tb[:1].view(np.uint8)).all(), "copies are not bit-equal rows"
        sg = np.ascontiguousarray(s[:, group])
        assert (sg.view(np.uint64) == sg[:, :1].view(np.uint64)).all(), "bit-equal rows with different reference scores"
        assert len({t[r].tobytes() for r in range(case.N)}) == case.N - case.copies + 1, "an unplanned duplicate row"
        in_group[group] = True
    m = min(case.k + 1, case.N)
    ws, wi = reference(case, m)
    wi = wi - case.id_base
    gap = ws[:, :-1] - ws[:, 1:]
    both = in_group[wi[:, :-1]] & in_group[wi[:, 1:]]
    for z in case.zero:
        assert not q[z].any() and not s[z].any()             # every score of a zero query is 0: one tie over the whole index
        both[z] = True
    assert (gap[both] == 0).all()
    if (~both).any():
        assert gap[~both].min() > 2 * tol, "%s: neighbours %.3e apart, 2 tol = %.3e" % (case.name, gap[~both].min(), 2 * tol)
    # the planted queries: the copies are their strict maxima (a unit row against itself, Cauchy-Schwarz) -- the expected
    # list is the lowest copy rows, or all of them and then others
    for p in case.planted[:8] + case.planted[-8:]:
        n = min(case.k, case.copies)
        assert np.array_equal(wi[p, :n], group[:n]), (case.name, p)
    for z in case.zero:
        assert np.array_equal(wi[z, :case.k], np.arange(case.k))
    if case.ordinary_below:
        # the copies are not collected for another query: its threshold is the k-th candidate less 2 * 2 (S + 2) 5.97e-8 |q||t|
        # (kth_bound_kernel; the k <= 16 pass subtracts less), far above a score below zero
        others = np.setdiff1d(np.arange(case.Q), case.planted)
        assert (s[others, group[0]] < 0).all() and (ws[others, case.k - 1] > 1e-2).all()
        assert case.copies > COLLECT_CAP
    if case.kind == "all_equal":
        # More tied rows than the call has candidates (choose_nsplit: 9 query blocks of 128, 188 tiles -> 8 splits x 16): some copy
        # is outside every list, its split's bound is the tie's own fp32 score, and rescore_kernel's `bound + eps < k-th
        # candidate` cannot hold for any query ...
        assert case.copies > 8 * 16 and (case.Q + 127) // 128 == 9 and (case.N + 31) // 32 == 188 and case.Q > SLOT_POOL
        assert case.copies + 64 < COLLECT_CAP                 # ... and a collect buffer takes them all
        assert int((s[0] >= ws[0, case.k - 1] - 1e-3).sum()) < COLLECT_CAP
    return True


def check(case, scores, ids):
    """The whole claim on one result.  Returns the worst |score - reference|."""
    ws, wi = expected(case)
    scores, ids = np.asarray(scores), np.asarray(ids)
    assert scores.shape == ws.shape and ids.shape == wi.shape, (scores.shape, ids.shape, ws.shape)
    assert scores.dtype == np.float64 and ids.dtype == np.int64
    bad = np.argwhere(ids != wi)
    assert bad.size == 0, "%s: %d ids differ, first at query %d rank %d: got %d, want %d" % (
        case.name, len(bad), bad[0][0], bad[0][1], ids[tuple(bad[0])], wi[tuple(bad[0])])
    err = np.abs(scores - ws)
    assert not np.isnan(scores).any()
    worst = float(err.max())
    assert worst <= score_bar(case), "%s: score off by %.3e, bar %.3e" % (case.name, worst, score_bar(case))
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "%s: a row id twice in one list" % case.name
    assert ((ids >= case.id_base) & (ids < case.id_base + case.N)).all(), "%s: a row id outside the index" % case.name
    d = scores[:, 1:] - scores[:, :-1]
    assert (d <= 0).all(), "%s: scores increase along a list" % case.name
    assert (ids[:, 1:] > ids[:, :-1])[d == 0].all(), "%s: an exact tie with the higher row first" % case.name
    return worst
