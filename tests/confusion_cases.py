"""Cases shared by tests/test_gpu_score_confusions.py (GPU) and tests/test_confusion_cases_host.py (CPU): sse_score_confusions,
the best k rows that are not among a query's positives and score at or above (its best positive's score) - margin.  DESIGN K6k.

One list, CASES.  Per case: inputs(case) builds queries, index and positives from the case's seed (the index and queries are
those of a tests/topk_cases.py case: its constructions of copies and planted queries are reused), reference(case) is the
float64 reference -- O.scores_f64, the best positive by (score descending, id ascending), the positives removed, the cut at
m - margin, O.topk, (-inf, INT64_MAX) padding, counts -- preconditions(case) proves the reference is one the device can be held
to, and check(case, scores, ids, counts, pos_scores, pos_ids) is what every entry point's result must pass.  The counter deltas
a call must cause:

  score_confusions_bruteforce_queries  +1 per query whose collect buffer (SSE_COLLECT_CAP = 4096 rows) overflowed: `brute`, exact
  score_confusions_collected_rows      every row of the answer was collected: at least the sum of the counts of the queries the
                                       float64 sweep did not take (`collected_min`)
  score_confusions_floor_queries       `floor`: exact where the case derives it (None: not derived, only >= 0)

No GPU import here."""
import functools

import numpy as np

from oracle import sse_oracle as O
from tests import topk_cases as TC
from tests.topk_cases import BASE, unit  # noqa: F401

COLLECT_CAP = TC.COLLECT_CAP
PAD_ID = np.iinfo(np.int64).max
INF = float("inf")


class Case:
    def __init__(self, name, base, k, margin, build, prepare=None, brute=0, floor=None, counts=None, why=""):
        self.name, self.base, self.k, self.margin, self.build, self.prepare = name, base, k, margin, build, prepare
        self.Q, self.N, self.S, self.id_base, self.upload = base.Q, base.N, base.S, base.id_base, base.upload
        self.brute = brute        # delta of score_confusions_bruteforce_queries per call
        self.floor = floor        # delta of score_confusions_floor_queries per call, None: not derived
        self.counts = counts      # the counts the case claims (None: whatever the reference says)
        self.why = why

    def __repr__(self):
        return self.name


def _base(name, Q, N, S, **kw):
    return TC.Case(name, Q, N, S, 1, seed=kw.pop("seed", 9000 + Q + N + S), **kw)


# ---- builders: (case, q, t, group, s) -> positives int64 [Q, n_pos], GLOBAL ids, -1 padded

def _ranked(s):
    return np.argsort(-s, axis=1, kind="stable")


def _b_rank(rank, n_pos=1):
    """the row at `rank` of every query's list; n_pos = 3: that row, padding, that row again"""
    def build(case, q, t, group, s):
        r = _ranked(s)[:, rank].astype(np.int64) + case.id_base
        if n_pos == 1:
            return r[:, None].copy()
        return np.stack([r, np.full_like(r, -1), r], axis=1)
    return build


def _b_mixed64(case, q, t, group, s):
    o = _ranked(s).astype(np.int64)
    pos = np.full((case.Q, 64), -1, np.int64)                 # -1 padding
    for qi in range(case.Q):
        pos[qi, 0:5] = o[qi, :5]                              # the five best rows ...
        pos[qi, 5:10] = o[qi, :5]                             # ... twice
        pos[qi, 10:14] = o[qi, 6:10]                          # (the sixth best stays)
        pos[qi, 20:24] = [case.N, case.N + 5, 2 ** 40, -case.N]   # outside the index
        pos[qi, 40:44] = o[qi, 10:14]
        pos[qi, 63] = o[qi, 30]
    return pos + np.where(pos == -1, 0, case.id_base)


def _b_shard(case, q, t, group, s):
    """query 0: all padding.  query 1: one positive, in the tail tile.  query 2: a real positive and the best row's LOCAL number,
    which is no id of this shard.  query 3: the third best row twice."""
    assert case.id_base > case.N and case.Q == 4
    o = _ranked(s).astype(np.int64)
    pos = np.full((4, 3), -1, np.int64)
    pos[1, 1] = case.N - 5 + case.id_base
    pos[2] = [o[2, 0], o[2, 4] + case.id_base, -1]
    pos[3] = [o[3, 2] + case.id_base, -1, o[3, 2] + case.id_base]
    return pos


def _b_copies(case, q, t, group, s):
    """two copies are the positives of every query (a tie among positives: the lower id is the best), the other copies score
    exactly m"""
    return np.tile(np.array([[group[7], group[3]]], np.int64) + case.id_base, (case.Q, 1))


def _b_overflow_below(case, q, t, group, s):
    """the planted query's positive is an ordinary row: the 4500 copies score above it.  Every other query's is its best row."""
    pos = _ranked(s)[:, :1].astype(np.int64)
    p = case.base.planted[0]
    pos[p, 0] = _ranked(np.where(np.isin(np.arange(case.N), group), -np.inf, s[p:p + 1]))[0, 0]
    return pos + case.id_base


PLANT_ROW = 5     # an ordinary row of the crowded construction (r % 4 == 1)


def _p_plant_above(case, q, t, group):
    t[PLANT_ROW] = 2.0 * t[group[0]]      # (exact in fp32) scores 2 for the planted query, twice the copies' below-zero score for the rest


def _b_overflow_above(case, q, t, group, s):
    pos = _ranked(s)[:, :1].astype(np.int64)
    assert pos[case.base.planted[0], 0] == PLANT_ROW
    return pos + case.id_base


_A = dict(Q=4, N=500, S=64)      # tail tile 15 * 32 + 20
CASES = [
    Case("best_row_margin0", _base("a", **_A), 17, 0.0, _b_rank(0), floor=4, counts=(0, 0, 0, 0),
         why="the positive is the overall best row: nothing above it, all padding; the floor is the stored threshold"),
    Case("three_above_margin0", _base("a", **_A), 17, 0.0, _b_rank(3, n_pos=3), counts=(3, 3, 3, 3),
         why="exactly 3 rows above the positive; n_pos = 3 with padding and a duplicate"),
    Case("margin_inf_n64", _base("a", **_A), 17, INF, _b_mixed64, floor=0, counts=(17,) * 4,
         why="no cut: the filtered reference with exclude = positives; n_pos = 64, duplicates, ids outside, padding"),
    Case("negative_margin", _base("a", **_A), 17, -0.05, _b_rank(9), why="the floor above the best positive"),
    Case("margin_tenth", _base("a", **_A), 17, 0.03, _b_rank(2), why="the common case: a few rows on either side of the positive"),
    Case("shard_base_dev", _base("b", upload="dev", id_base=BASE, **_A), 17, 0.03, _b_shard,
         why="ids global; a row of positives that is all padding (no cut); a positive in the tail tile; an id of another shard"),
    Case("s50_f64_k1", _base("c", 4, 500, 50, upload="f64"), 1, 0.05, _b_rank(2), counts=(1, 1, 1, 1),
         why="float64 index: the idx64 branch of the dot, in the floor kernel too; k = 1"),
    Case("k1024_over_n", _base("a", **_A), 1024, 0.3, _b_rank(0), why="k > N, a floor that keeps a hundred rows"),
    Case("k1024_over_n_inf", _base("a", **_A), 1024, INF, _b_rank(0), floor=0, counts=(499,) * 4, why="k > N, every other row"),
    Case("copies_on_floor", TC.Case("ct", 9, 2000, 32, 1, kind="tie", seed=11, copies=30, planted=(4,)), 40, 0.0, _b_copies,
         why="28 copies score exactly m: all are confusions (>=), in id order; the best of two tied positives is the lower id"),
    Case("overflow_floor_below", TC.Case("co", 8, 6000, 64, 1, kind="dup", seed=14, copies=4500, planted=(3,), ordinary_below=True),
         50, 0.0, _b_overflow_below, brute=1, counts=(0, 0, 0, 50, 0, 0, 0, 0),
         why="4500 copies above the floor > 4096: the float64 sweep serves the planted query alone"),
    Case("overflow_positive_above", TC.Case("co", 8, 6000, 64, 1, kind="dup", seed=14, copies=4500, planted=(3,), ordinary_below=True),
         50, 0.0, _b_overflow_above, prepare=_p_plant_above, brute=0, floor=8, counts=(0,) * 8,
         why="a positive above the copies: the floor keeps them out of the buffer, no float64 sweep"),
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(q, t, group, s, pos): read-only arrays; s = O.scores_f64 [Q, N], pos int64 [Q, n_pos]."""
    q0, t0, group = TC.inputs(case.base)
    q, t = q0.copy(), t0.copy()
    if case.prepare:
        case.prepare(case, q, t, group)
    s = _scores(case, q, t, group)
    pos = np.ascontiguousarray(case.build(case, q, t, group, s), dtype=np.int64)
    d = dict(q=q, t=t, group=group, s=s, pos=pos)
    for v in d.values():
        v.setflags(write=False)
    return d


def _scores(case, q, t, group):
    """O.scores_f64; bit-equal rows get ONE reference score (the construction of topk_cases.reference_scores)."""
    t64 = np.asarray(t, np.float64)
    if group.size:
        keep = np.ones(case.N, bool)
        keep[group[1:]] = False
        col = np.cumsum(keep) - 1
        col[group] = col[group[0]]
        return np.ascontiguousarray(O.scores_f64(q, t64[keep])[:, col])
    return np.ascontiguousarray(O.scores_f64(q, t64))


@functools.lru_cache(maxsize=None)
def positive_rows(case):
    """per query the sorted local rows of P(q): the in-range entries, each once"""
    pos = inputs(case)["pos"]
    out = []
    for qi in range(case.Q):
        r = pos[qi] - case.id_base
        out.append(np.unique(r[(pos[qi] >= case.id_base) & (r < case.N)]))
    return out


@functools.lru_cache(maxsize=None)
def best_positive(case):
    """(m float64 [Q], b int64 [Q] global, f float64 [Q])"""
    s = inputs(case)["s"]
    m = np.full(case.Q, -np.inf)
    b = np.full(case.Q, PAD_ID, np.int64)
    for qi, rows in enumerate(positive_rows(case)):
        if rows.size:
            j = np.lexsort((rows, -s[qi, rows]))[0]          # score descending, then id ascending
            m[qi], b[qi] = s[qi, rows[j]], rows[j] + case.id_base
    with np.errstate(invalid="ignore"):
        f = m - np.float64(case.margin)
    for a in (m, b, f):
        a.setflags(write=False)
    return m, b, f


@functools.lru_cache(maxsize=None)
def confusions(case, cut=True):
    """[Q, N] truth table: not a positive and (cut) at or above the floor"""
    s = inputs(case)["s"]
    e = np.ones((case.Q, case.N), bool)
    for qi, rows in enumerate(positive_rows(case)):
        e[qi, rows] = False
    if cut:
        e &= s >= best_positive(case)[2][:, None]
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def reference(case, k=None, cut=True):
    """(scores float64 [Q,k], ids int64 [Q,k], counts int32 [Q], pos_scores [Q], pos_ids [Q]), read-only.  cut=False: the
    filtered reference with exclude = positives."""
    k = case.k if k is None else k
    s, e = inputs(case)["s"], confusions(case, cut)
    ws = np.full((case.Q, k), -np.inf)
    wi = np.full((case.Q, k), PAD_ID, np.int64)
    cnt = np.zeros(case.Q, np.int32)
    for qi in range(case.Q):
        cols = np.flatnonzero(e[qi])
        c = min(k, cols.size)
        cnt[qi] = c
        if c:
            ss, ii = O.topk(s[qi:qi + 1, cols], c)
            ws[qi, :c], wi[qi, :c] = ss[0], cols[ii[0]] + case.id_base
    for a in (ws, wi, cnt):
        a.setflags(write=False)
    m, b, _ = best_positive(case)
    return ws, wi, cnt, m, b


def expected(case):
    return reference(case)


def scales(case):
    I = inputs(case)
    qn = float(np.linalg.norm(I["q"].astype(np.float64), axis=1).max())
    tn = float(np.linalg.norm(np.asarray(I["t"], np.float64), axis=1).max())
    return qn, tn, 2.0 * case.S * 2.0 ** -53 * qn * tn


def score_bar(case):
    """topk_cases.score_bar on this case's arrays."""
    qn, tn, tol = scales(case)
    return max(1e-12 * qn * tn, tol)


def collected_min(case):
    """every answer row of a query the float64 sweep did not take was collected"""
    cnt = reference(case)[2].astype(np.int64)
    if case.brute:
        cnt = np.delete(cnt, list(case.base.planted))
    return int(cnt.sum())


def preconditions(case):
    """AssertionError unless the reference is one a device summing in its own order must reproduce id for id: the device's m and
    a row's score each differ from the reference's by at most the bar, so a row decides the same way on both sides of the floor
    when it is further than twice the bar from it -- or sits on it exactly, as a bit-equal copy of the best positive with margin 0."""
    I = inputs(case)
    q, t, group, s, pos = I["q"], I["t"], I["group"], I["s"], I["pos"]
    bar = score_bar(case)
    assert q.shape == (case.Q, case.S) and t.shape == (case.N, case.S) and 1 <= case.k <= 1024
    assert pos.shape[0] == case.Q and 1 <= pos.shape[1] <= 64
    assert case.margin == case.margin and case.margin > -INF
    in_group = np.zeros(case.N, bool)
    if group.size:
        tb = np.ascontiguousarray(t[group])
        assert (tb.view(np.uint8) == tb[:1].view(np.uint8)).all(), "copies are not bit-equal rows"
        assert len({t[r].tobytes() for r in range(case.N)}) == case.N - group.size + 1, "an unplanned duplicate row"
        in_group[group] = True
    m, b, f = best_positive(case)
    notpos = confusions(case, cut=False)
    for qi, rows in enumerate(positive_rows(case)):
        if not rows.size:
            assert m[qi] == -np.inf and b[qi] == PAD_ID and f[qi] == -np.inf
            continue
        # the best positive leads the next by more than the bar, unless they are bit-equal copies
        brow = b[qi] - case.id_base
        for r in rows:
            if r != brow and not (in_group[r] and in_group[brow]):
                assert m[qi] - s[qi, r] > 2 * bar, (case.name, qi, "two positives within the bar")
        # no non-positive row within the bar of the floor
        if np.isfinite(f[qi]):
            d = np.abs(s[qi] - f[qi])
            on_floor = notpos[qi] & (d <= 2 * bar + 1e-15)
            if case.margin == 0.0 and in_group[brow]:
                assert (s[qi, on_floor] == m[qi]).all() and in_group[np.flatnonzero(on_floor)].all(), (case.name, qi)
            else:
                assert not on_floor.any(), (case.name, qi, "a row within the bar of the floor")
    ws, wi, cnt, _, _ = reference(case, min(case.k + 1, 1025))
    for qi in range(case.Q):
        c = int(cnt[qi])
        if c < 2:
            continue
        rows = wi[qi, :c] - case.id_base
        gap = ws[qi, :c - 1] - ws[qi, 1:c]
        both = in_group[rows[:-1]] & in_group[rows[1:]]
        assert (gap[both] == 0).all()
        if (~both).any():
            assert gap[~both].min() > 2 * bar, "%s query %d: neighbours %.3e apart, 2 bar = %.3e" % (case.name, qi, gap[~both].min(), 2 * bar)
    want = reference(case)[2]
    assert np.array_equal(want, np.minimum(confusions(case).sum(1), case.k))
    if case.counts is not None:
        assert tuple(int(c) for c in want) == tuple(case.counts), (case.name, want)
    if case.margin == INF:      # must equal the filtered reference with exclude = positives
        for a, w in zip(reference(case)[:3], reference(case, cut=False)[:3]):
            assert np.array_equal(a, w)
        assert (f == -np.inf).all()
    elif case.counts is None:   # the cut does something, and leaves something
        uncut = reference(case, cut=False)[2]
        assert (want < uncut).any() and want.any(), (case.name, want)
    # overflow: the collect threshold is at most the fp32 score of every answer row; a buffer takes SSE_COLLECT_CAP rows
    fp32_bound = 2.0 * (case.S + 2) * 5.97e-8 * scales(case)[0] * scales(case)[1]
    if case.brute == 0:
        if case.N > COLLECT_CAP:
            # the floor is the stored threshold of every query and keeps all but a few rows out of the buffer
            assert case.floor == case.Q
            assert ((s >= f[:, None] - 2 * fp32_bound).sum(1) < 64).all()
    else:
        planted = list(case.base.planted)
        assert len(planted) == case.brute and case.base.ordinary_below and group.size > COLLECT_CAP
        for p in planted:
            # the copies are bit-equal in any arithmetic, above the floor and not positives: all of them are at or above any
            # threshold that keeps the k answer rows, which are copies themselves
            assert (s[p, group] > f[p] + 2 * bar).all() and notpos[p, group].all()
            assert np.array_equal(wi[p, :case.k] - case.id_base, group[:case.k])
        for o in np.setdiff1d(np.arange(case.Q), planted):
            # another query's floor is its best row's score, above zero; the copies score below zero
            assert s[o, group[0]] < 0 and f[o] > 1e-2 and int((s[o] >= f[o] - 2 * fp32_bound).sum()) < 64
    if case.floor == case.Q:
        # flo = rd(f - e) wins over rd(theta - 2 e): theta, the (k + n_pos)-th largest of maxima over disjoint row sets, is at most
        # the second best score of the query, which is further below f than the fp32 bound
        assert case.k + pos.shape[1] >= 2
        second = np.sort(s, axis=1)[:, -2]
        assert (f - second > 4 * fp32_bound).all(), case.name
    if case.floor == 0:
        assert (f == -np.inf).all()
    return True


def check(case, scores, ids, counts, pos_scores, pos_ids):
    """The whole claim on one result.  Returns the worst |score - reference| over the real entries and the best positives."""
    ws, wi, wc, wm, wb = expected(case)
    scores, ids, counts, pos_scores, pos_ids = (np.asarray(a) for a in (scores, ids, counts, pos_scores, pos_ids))
    assert scores.shape == ws.shape and ids.shape == wi.shape and counts.shape == wc.shape, (scores.shape, ids.shape, counts.shape)
    assert pos_scores.shape == wm.shape and pos_ids.shape == wb.shape
    assert scores.dtype == np.float64 and ids.dtype == np.int64 and counts.dtype == np.int32
    assert pos_scores.dtype == np.float64 and pos_ids.dtype == np.int64
    assert np.array_equal(pos_ids, wb), "%s: best positive ids %s, want %s" % (case.name, pos_ids.tolist()[:16], wb.tolist()[:16])
    none = wb == PAD_ID
    assert (pos_scores[none] == -np.inf).all() and not np.isnan(pos_scores).any()
    worst = float(np.abs(pos_scores[~none] - wm[~none]).max()) if (~none).any() else 0.0
    assert np.array_equal(counts, wc), "%s: counts %s, want %s" % (case.name, counts.tolist()[:16], wc.tolist()[:16])
    real = np.arange(case.k)[None, :] < wc[:, None]
    assert (ids[~real] == PAD_ID).all() and np.array_equal(scores[~real], np.full(int((~real).sum()), -np.inf)), \
        "%s: a padding slot holds something else than (-inf, INT64_MAX)" % case.name
    rows = ids - case.id_base
    inside = (rows >= 0) & (rows < case.N)
    assert inside[real].all(), "%s: a row id outside the index" % case.name
    qq = np.broadcast_to(np.arange(case.Q)[:, None], ids.shape)
    assert confusions(case, cut=False)[qq[real], rows[real]].all(), "%s: a positive in a result" % case.name
    assert confusions(case)[qq[real], rows[real]].all(), "%s: a row below the floor in a result" % case.name
    bad = np.argwhere(ids != wi)
    assert bad.size == 0, "%s: %d ids differ, first at query %d rank %d: got %d, want %d" % (
        case.name, len(bad), bad[0][0], bad[0][1], ids[tuple(bad[0])], wi[tuple(bad[0])])
    assert not np.isnan(scores).any()
    if real.any():
        worst = max(worst, float(np.abs(scores[real] - ws[real]).max()))
    assert worst <= score_bar(case), "%s: score off by %.3e, bar %.3e" % (case.name, worst, score_bar(case))
    # the returned rows are at or above the returned floor, bit for bit
    with np.errstate(invalid="ignore"):
        got_f = pos_scores - np.float64(case.margin)
    assert (scores >= got_f[:, None])[real].all(), "%s: a returned score below the returned floor" % case.name
    for qi in range(case.Q):
        c = int(wc[qi])
        assert len(set(ids[qi, :c].tolist())) == c, "%s: a row id twice in one list" % case.name
        if c < 2:
            continue
        d = scores[qi, 1:c] - scores[qi, :c - 1]
        assert (d <= 0).all(), "%s: scores increase along a list" % case.name
        assert (ids[qi, 1:c] > ids[qi, :c - 1])[d == 0].all(), "%s: an exact tie with the higher row first" % case.name
    return worst


# ---- the same reference on any score matrix (tests/test_gpu_hard_learning.py: a model's own encodings)

def reference_arrays(s, pos, margin, k, id_base=0):
    """reference() on a float64 score matrix s [Q, N] and positives pos int64 [Q, n_pos] (global ids, -1 padded):
    (scores [Q,k], ids [Q,k], counts int32 [Q], pos_scores [Q], pos_ids [Q])."""
    Q, N = s.shape
    ws, wi, cnt = np.full((Q, k), -np.inf), np.full((Q, k), PAD_ID, np.int64), np.zeros(Q, np.int32)
    m, b = np.full(Q, -np.inf), np.full(Q, PAD_ID, np.int64)
    for qi in range(Q):
        r = pos[qi] - id_base
        rows = np.unique(r[(pos[qi] >= id_base) & (r < N)])
        ok = np.ones(N, bool)
        ok[rows] = False
        if rows.size:
            j = np.lexsort((rows, -s[qi, rows]))[0]
            m[qi], b[qi] = s[qi, rows[j]], rows[j] + id_base
        with np.errstate(invalid="ignore"):
            cols = np.flatnonzero(ok & (s[qi] >= m[qi] - np.float64(margin)))
        c = min(k, cols.size)
        cnt[qi] = c
        if c:
            ss, ii = O.topk(s[qi:qi + 1, cols], c)
            ws[qi, :c], wi[qi, :c] = ss[0], cols[ii[0]] + id_base
    return ws, wi, cnt, m, b


def rows_decidable(s, pos, margin, k, bar, same):
    """bool [Q]: the queries whose reference a device summing in its own order must reproduce id for id -- the three rules of
    preconditions(), per query.  same[r]: a label equal for bit-equal index rows (they are exempt among themselves: their
    scores are equal bits on any device, and must be in s)."""
    Q, N = s.shape
    ws, wi, cnt, m, b = reference_arrays(s, pos, margin, min(k + 1, N))
    good = np.ones(Q, bool)
    for qi in range(Q):
        rows = np.unique(pos[qi][(pos[qi] >= 0) & (pos[qi] < N)])
        if not rows.size:
            continue
        oth = rows[same[rows] != same[b[qi]]]
        if oth.size and (m[qi] - s[qi, oth]).min() <= 2 * bar:
            good[qi] = False
        f = m[qi] - np.float64(margin)
        if np.isfinite(f):
            near = np.abs(s[qi] - f) <= 2 * bar + 1e-15
            near[rows] = False
            if margin == 0.0:
                near &= ~((same == same[b[qi]]) & (s[qi] == m[qi]))
            if near.any():
                good[qi] = False
        c = int(cnt[qi])
        if c >= 2:
            r = wi[qi, :c]
            gap = ws[qi, :c - 1] - ws[qi, 1:c]
            twins = same[r[:-1]] == same[r[1:]]
            if (gap[twins] != 0).any() or (gap[~twins] <= 2 * bar).any():
                good[qi] = False
    return good
