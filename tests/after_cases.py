"""Cases shared by tests/test_gpu_score_after.py (GPU) and tests/test_after_cases_host.py (CPU): sse_score_topk_after, the exact
next k rows of score_topk's ranked list after a (score, id) cursor, among the tag-eligible rows.  DESIGN K6j.

One list, CASES, on tests/topk_cases.py bases.  A case is an index, queries, (optionally) tags and masks, and a list of STEPS:
one call each, with k and one cursor per query.  inputs(case) builds the arrays from the case's seed, expected(case, step) is
the float64 reference, preconditions(case) proves the reference is one the device can be held to, check(case, step, scores, ids,
counts) is what every entry point's result must pass.

The rule for cursors.  The device's score64 and the oracle's differ by summation order (tol = 2 S 2^-53 |q| |t|), so a cursor
score is one of two kinds only, and a cursor is written in RANK space (positions of the query's full float64 ranking):
  ("dev", j, id)   the score the DEVICE returned for the row at full rank j in an earlier step of the same case; id None: that
                   row's id, else the given global id (ties, copies, foreign ids).  cursor_arrays() looks the score up in
                   what the earlier steps returned (`known`); preconditions() proves the row was returned by then.
  ("mid", j, id)   the midpoint of the reference scores at full ranks j and j + 1, which preconditions() proves to be more
                   than 4 tol apart: at least 2 tol from every score of the query, on the device too.  id is arbitrary.
  ("inf",) ("ninf",) ("nan",) ("below", id)   +inf: everything is after it; -inf, NaN: nothing; below: a finite score under
                   every score of the query.
A step whose `cursors` is None hands no cursor arrays at all (both NULL).  In rank space the rows after a cursor are known
without the device: after a "mid" or "dev" cursor come the rows of lower reference score and -- "dev" only -- the bit-equal
copies of row j with a higher id than the cursor's (preconditions: reference scores closer than 2 tol are bit-equal copies).

The counter deltas a call must cause: score_after_bruteforce_queries exactly step.brute, score_after_collected_rows at least
the answer rows of the queries the float64 sweep did not take.

No GPU import here."""
import functools

import numpy as np

from oracle import sse_oracle as O
from tests import filtered_cases as FC
from tests import topk_cases as TC
from tests.topk_cases import BASE, unit  # noqa: F401

COLLECT_CAP = TC.COLLECT_CAP
PAD_ID = FC.PAD_ID
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
bit = FC.bit
BAND = 200                 # rows of the band case


class Step:
    def __init__(self, label, k, cursors, brute=0, planted=()):
        self.label, self.k, self.cursors, self.brute = label, k, cursors, brute
        self.planted = tuple(planted)     # the queries the float64 sweep serves (len == brute)

    def __repr__(self):
        return self.label


class Case:
    def __init__(self, name, base, build, steps, edit=None, variants=None, tag_entry="host", first_page=False, why=""):
        self.name, self.base, self.build, self.make_steps, self.edit = name, base, build, steps, edit
        self.Q, self.N, self.S, self.id_base, self.upload = base.Q, base.N, base.S, base.id_base, base.upload
        self.variants = variants or (("default", 1),)   # (label, score_filtered_skip): results equal across them
        self.tag_entry = tag_entry
        self.first_page = first_page      # the GPU test also compares step 0 with score_topk and score_topk_filtered
        self.why = why

    def __repr__(self):
        return self.name


def _base(name, Q, N, S, **kw):
    return TC.Case(name, Q, N, S, 1, seed=kw.pop("seed", 9000 + Q + N + S), **kw)


# ---- inputs

@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(q, t, group, s, tags, any, none, band): arrays or None, read-only"""
    q0, t0, group = TC.inputs(case.base)
    q, t = q0.copy(), t0.copy()
    rng = np.random.RandomState(case.base.seed + 99)
    d = dict(tags=None, any=None, none=None, band=None)
    if case.edit is not None:
        d.update(case.edit(case, q, t, rng))
    s = FC._scores(case, q, t, group)
    d.update(case.build(case, q, t, group, s, rng))
    assert d.get("exclude") is None
    d.update(q=q, t=t, group=group, s=s)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def order(case):
    """[Q, N] rows of every query in score_topk's order: reference score descending, equal scores by ascending row"""
    o = np.argsort(-inputs(case)["s"], axis=1, kind="stable")
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def eligible(case):
    I = inputs(case)
    e = np.ones((case.Q, case.N), bool)
    if I["tags"] is not None:
        tg = I["tags"][None, :]
        if I["any"] is not None:
            e &= (I["any"][:, None] == 0) | ((tg & I["any"][:, None]) != 0)
        if I["none"] is not None:
            e &= (tg & I["none"][:, None]) == 0
    e.setflags(write=False)
    return e


def elig_rank(case, qi, j):
    """full rank of query qi's j-th eligible row (0-based)"""
    o = order(case)[qi]
    return int(np.flatnonzero(eligible(case)[qi, o])[j])


def scales(case):
    I = inputs(case)
    qn = float(np.linalg.norm(I["q"].astype(np.float64), axis=1).max())
    tn = float(np.linalg.norm(np.asarray(I["t"], np.float64), axis=1).max())
    return qn, tn, 2.0 * case.S * 2.0 ** -53 * qn * tn


def score_bar(case):
    qn, tn, tol = scales(case)
    return max(1e-12 * qn * tn, tol)


@functools.lru_cache(maxsize=None)
def steps(case):
    return tuple(case.make_steps(case))


def cursors_of(case, step):
    """one cursor per query, or None"""
    if step.cursors is None:
        return None
    c = step.cursors
    if isinstance(c, tuple) and c and isinstance(c[0], str):
        c = [c] * case.Q
    assert len(c) == case.Q
    return list(c)


# ---- the reference

def after_mask(case, step):
    """[Q, N] bool: row is after the query's cursor, decided in rank space"""
    I = inputs(case)
    s, o = I["s"], order(case)
    cur = cursors_of(case, step)
    m = np.ones((case.Q, case.N), bool)
    if cur is None:
        return m
    for qi, c in enumerate(cur):
        kind = c[0]
        if kind == "inf":
            continue
        if kind in ("ninf", "nan", "below"):
            m[qi] = False
        elif kind == "mid":
            m[qi] = False
            m[qi, o[qi, c[1] + 1:]] = True
        elif kind == "dev":
            row = o[qi, c[1]]
            cid = case.id_base + int(row) if c[2] is None else int(c[2])
            ids = case.id_base + np.arange(case.N, dtype=np.int64)
            m[qi] = (s[qi] < s[qi, row]) | ((s[qi] == s[qi, row]) & (ids > cid))
        else:
            raise AssertionError(c)
    return m


def expected(case, step):
    """(scores float64 [Q,k], ids int64 [Q,k], counts int32 [Q])"""
    s, o = inputs(case)["s"], order(case)
    ok = eligible(case) & after_mask(case, step)
    k = step.k
    ws = np.full((case.Q, k), -np.inf)
    wi = np.full((case.Q, k), PAD_ID, np.int64)
    wc = np.zeros(case.Q, np.int32)
    for qi in range(case.Q):
        rows = o[qi][ok[qi, o[qi]]][:k]
        c = rows.size
        ws[qi, :c], wi[qi, :c], wc[qi] = s[qi, rows], rows + case.id_base, c
    return ws, wi, wc


def cursor_arrays(case, step, known):
    """(scores float64 [Q], ids int64 [Q]) as handed to the call, or None.  known[qi]: {global id: device score} of every entry
    the earlier steps returned for query qi."""
    cur = cursors_of(case, step)
    if cur is None:
        return None
    s, o = inputs(case)["s"], order(case)
    cs = np.zeros(case.Q, np.float64)
    ci = np.zeros(case.Q, np.int64)
    for qi, c in enumerate(cur):
        kind = c[0]
        if kind in ("inf", "ninf", "nan"):
            cs[qi], ci[qi] = {"inf": np.inf, "ninf": -np.inf, "nan": np.nan}[kind], 0
        elif kind == "below":
            cs[qi], ci[qi] = s[qi].min() - 1.0, c[1]
        elif kind == "mid":
            a, b = s[qi, o[qi, c[1]]], s[qi, o[qi, c[1] + 1]]
            cs[qi], ci[qi] = b + (a - b) / 2, c[2]
        else:
            rid = case.id_base + int(o[qi, c[1]])
            assert rid in known[qi], "%s %s query %d: the device has not returned row %d yet" % (case.name, step.label, qi, rid)
            cs[qi], ci[qi] = known[qi][rid], rid if c[2] is None else c[2]
    return cs, ci


def learn(known, scores, ids, counts):
    for qi in range(len(known)):
        for j in range(int(counts[qi])):
            known[qi][int(ids[qi, j])] = float(scores[qi, j])


def oracle_known(case, upto):
    """`known` as the oracle would fill it over steps [0, upto): the reference scores stand in for the device's"""
    known = [dict() for _ in range(case.Q)]
    for st in steps(case)[:upto]:
        learn(known, *expected(case, st))
    return known


def collected_min(case, step):
    cnt = expected(case, step)[2].astype(np.int64)
    if step.brute:
        cnt = np.delete(cnt, list(step.planted))
    return int(cnt.sum())


# ---- builders (tags) and edits (rows)

def _b_none(case, q, t, group, s, rng):
    return {}


def _b_sorted(case, q, t, group, s, rng):
    d = FC._b_sorted(case, q, t, group, s, rng)
    return d


def _e_band(case, q, t, rng):
    """BAND rows that are row 100 with component d moved by 1, 2, ... BAND ulps (each one ulp from the one before), spread over
    the index; query 0 is the base row itself.  d: the component of the base row of largest magnitude whose BAND ulps stay
    inside its binade."""
    b = t[100].copy()
    d = int(np.argmax(np.abs(b)))
    rows = 300 + 8 * np.arange(BAND) + (np.arange(BAND) % 5)       # up to 1896, every phase of a tile
    step_to = np.float32(np.inf) if b[d] > 0 else np.float32(-np.inf)
    v = b[d]
    for r in rows:
        v = np.nextafter(v, step_to)                                # one ulp further from zero
        t[r] = b
        t[r, d] = v
    q[0] = b
    return dict(band=rows.astype(np.int64))


# ---- steps

def _page(label, case, page, k, **kw):
    """cursor of page `page` (0-based) of size k in every query's ELIGIBLE list: the device's (score, id) of its last entry of
    the page before; a query with fewer entries than that gets the last it has"""
    if page == 0:
        return Step(label, k, ("inf",), **kw)
    cur = []
    for qi in range(case.Q):
        n = int(eligible(case)[qi].sum())
        cur.append(("dev", elig_rank(case, qi, min(page * k, n) - 1), None))
    return Step(label, k, cur, **kw)


def _s_first(k):
    return lambda case: [Step("inf", k, ("inf",)), Step("null", k, None)]


def _s_chain(k):
    def make(case):
        pages = (case.N + k - 1) // k
        return [_page("page%d" % p, case, p, k) for p in range(pages + 1)]
    return make


def _s_pages(k, n=2):
    return lambda case: [_page("page%d" % p, case, p, k) for p in range(n)]


def _s_ties(case):
    group = inputs(case)["group"]
    p = case.base.planted[0]
    between = int(group[9]) + 1
    assert between not in set(group.tolist()) and group[9] < between < group[10]

    def cur(idv):
        # the planted query: the copies' score (full rank 0, returned by the first step) with the id under test; the others:
        # their own tenth row
        return [("dev", 0, idv) if qi == p else ("dev", 9, None) for qi in range(case.Q)]
    b = case.id_base
    return [Step("first", 20, ("inf",)),
            Step("tenth_copy", 40, cur(b + int(group[9]))),
            Step("between_two_copies", 40, cur(b + between)),
            Step("int64_max", 40, cur(I64_MAX)),
            Step("int64_min", 40, cur(I64_MIN))]


def _s_band(case):
    I = inputs(case)
    o = order(case)
    cur = []
    for qi in range(case.Q):
        pos = np.flatnonzero(np.isin(o[qi], I["band"]))            # full ranks of the band rows
        cur.append(("mid", int(pos[BAND // 2 - 1]), 77 + qi))       # between the 100th and the 101st of them
    return [Step("mid_of_band", 150, cur)]


def _s_between(case):
    ids = [12345, -1, case.id_base + case.N + 5, 0, I64_MAX, I64_MIN, case.id_base, case.id_base + 600, 2 ** 40]
    return [Step("mid_foreign_ids", 33, [("mid", 50 + 7 * qi, ids[qi]) for qi in range(case.Q)])]


def _s_few(case):
    N = case.N
    return [Step("leaves_3", 10, ("mid", N - 4, 5)),
            Step("leaves_1", 10, ("mid", N - 2, 5)),
            Step("leaves_0", 10, ("below", 5)),
            Step("nan", 10, ("nan",)),
            Step("ninf", 10, ("ninf",)),
            Step("mixed", 10, [("inf",), ("mid", 400, 1), ("nan",), ("mid", 250, 2)])]


def _s_tags_best_ineligible(case):
    # the unfiltered top 100 of every query are ineligible: a cursor in the middle of them changes nothing
    return [_page("page0", case, 0, 20), _page("page1", case, 1, 20), Step("mid_inside_ineligible", 20, ("mid", 50, 9))]


def _s_k1024(case):
    return [Step("first", 1024, ("inf",)), Step("second", 1024, ("dev", 1023, None))]


def _s_overflow(case):
    group = inputs(case)["group"]
    p = case.base.planted[0]
    cid = case.id_base + int(group[1999])                          # the 2000th copy
    cur = [("dev", 0, cid) if qi == p else ("dev", 49, None) for qi in range(case.Q)]
    return [Step("first", 50, ("inf",), brute=1, planted=(p,)), Step("inside_the_copies", 50, cur, brute=1, planted=(p,))]


_TWO = FC._b_one_of(4, two=True)

CASES = [
    Case("first_page_k10", _base("fp", 5, 3000, 32, seed=7101), _b_none, _s_first(10), first_page=True, why="+inf and NULL: score_topk's bits, k <= 16"),
    Case("first_page_k40", _base("fp", 5, 3000, 32, seed=7101), _b_none, _s_first(40), first_page=True, why="+inf and NULL: score_topk's bits, k > 16"),
    Case("chain_k33", _base("ch", 5, 700, 32), _b_none, _s_chain(33), why="22 pages to the end (tail tile of 28 rows), last count 7, then 0"),
    Case("ties", TC.Case("at", 9, 2000, 32, 20, kind="tie", seed=11, copies=30, planted=(4,)), _b_none, _s_ties,
         why="the cursor inside 30 equal scores: the id decides"),
    Case("band", _base("bd", 3, 2000, 32, seed=9301), _b_none, _s_band, edit=_e_band,
         why="200 rows within the fp32 bound of each other, the cursor between them: float64 decides"),
    Case("between_dev_base", _base("bb", 9, 1200, 40, seed=7111, upload="dev", id_base=BASE), _b_none, _s_between, why="midpoint cursors, foreign ids, index_set_dev"),
    Case("between_f64_base", _base("bb", 9, 1200, 40, seed=7111, upload="f64", id_base=BASE), _b_none, _s_between, why="float64 index: idx64 branch"),
    Case("few_left", _base("fl", 4, 500, 16), _b_none, _s_few, why="3, 1, 0 rows left; NaN, -inf; cursors mixed in one call"),
    Case("tags_one_of_eight", _base("o8", 5, 3000, 32), FC._b_one_of(8), _s_pages(10), why="page 2 among the eligible rows"),
    Case("tags_best_rows_ineligible", _base("bi", 9, 2000, 32), FC._b_best_ineligible, _s_tags_best_ineligible, why="maxima from eligible rows only"),
    Case("tags_sorted", _base("st", 64, 4096, 32), _b_sorted, _s_pages(10), variants=(("skip_on", 1), ("skip_off", 0)),
         why="tile skip on and off: equal results"),
    Case("q33_nq4", _base("n4", 33, 700, 64), _TWO, _s_pages(40), why="NQ = 4, partial second query tile"),
    Case("s300_nq2", _base("n2", 40, 700, 300), _TWO, _s_pages(40), why="NQ = 2"),
    Case("s620_nq1", _base("n1", 40, 700, 620), _TWO, _s_pages(40), why="NQ = 1 with Q > 32"),
    Case("k1024", _base("k1", 3, 5000, 64), _b_none, _s_k1024, why="largest k: rows 1025 .. 2048"),
    Case("overflow", TC.Case("ao", 8, 6000, 64, 50, kind="dup", seed=14, copies=4500, planted=(3,), ordinary_below=True), _b_none,
         _s_overflow, why="the cursor inside 4500 copies > 4096: the float64 sweep serves the planted query alone"),
    Case("folded_splits", _base("fs", 5, 16400, 16), FC._b_sixteen_blocks, _s_pages(10),
         why="513 tiles, 5 queries: 32 index splits share 16 x 256 maxima slots (atomicMax), eligible rows on both sides of a fold"),
]
BY_NAME = {c.name: c for c in CASES}


# ---- what the cases rest on

def preconditions(case):
    """AssertionError unless every cursor obeys the rule above, the reference is one a device summing in its own order must
    reproduce id for id, and every overflow is the one the case claims."""
    I = inputs(case)
    q, t, group, s = I["q"], I["t"], I["group"], I["s"]
    o = order(case)
    tol = scales(case)[2]
    assert q.shape == (case.Q, case.S) and t.shape == (case.N, case.S)
    in_group = np.zeros(case.N, bool)
    if group.size:
        tb = np.ascontiguousarray(t[group])
        assert (tb.view(np.uint8) == tb[:1].view(np.uint8)).all(), "copies are not bit-equal rows"
        in_group[group] = True
    assert len({t[r].tobytes() for r in range(case.N)}) == case.N - max(group.size, 1) + 1, "an unplanned duplicate row"
    # neighbours of the WHOLE ranking (a cursor may stand anywhere): bit-equal copies tie exactly, everything else is more than 2 tol apart
    ss = np.take_along_axis(s, o, 1)
    gap = ss[:, :-1] - ss[:, 1:]
    both = in_group[o[:, :-1]] & in_group[o[:, 1:]]
    assert (gap[both] == 0).all()
    assert gap[~both].min() > 2 * tol, "%s: neighbours %.3e apart, 2 tol = %.3e" % (case.name, gap[~both].min(), 2 * tol)
    known = [set() for _ in range(case.Q)]
    for st in steps(case):
        assert 1 <= st.k <= 1024
        cur = cursors_of(case, st)
        for qi, c in enumerate(cur or []):
            if c[0] == "mid":
                assert 0 <= c[1] < case.N - 1 and gap[qi, c[1]] > 4 * tol, (case.name, st.label, qi, gap[qi, c[1]], 4 * tol)
            elif c[0] == "dev":
                assert case.id_base + int(o[qi, c[1]]) in known[qi], "%s %s query %d: a device score no earlier step returns" % (case.name, st.label, qi)
            else:
                assert c[0] in ("inf", "ninf", "nan", "below")
        ws, wi, wc = expected(case, st)
        for qi in range(case.Q):
            known[qi].update(wi[qi, :wc[qi]].tolist())
        _overflow_preconditions(case, st)
    if I["band"] is not None:
        _band_preconditions(case)
    return True


def _eps32(case):
    """score_eps32 of the library: |fp32 score - score64| <= 2 (S + 2) 5.97e-8 |t|max |q|"""
    return 2.0 * (case.S + 2) * 5.97e-8 * scales(case)[1]


def _band_preconditions(case):
    I = inputs(case)
    s, rows, tol = I["s"], I["band"], scales(case)[2]
    assert rows.size == BAND and len(set(rows.tolist())) == BAND and 100 not in rows
    d = np.flatnonzero(I["t"][rows[0]] != I["t"][100])
    assert d.size == 1
    col = I["t"][np.concatenate([[100], rows]), d[0]]
    assert (np.diff(col.view(np.int32)) == np.sign(np.diff(col.view(np.int32))[0])).all(), "one ulp from row to row"
    other = np.delete(np.arange(case.S), d[0])
    assert (I["t"][rows][:, other] == I["t"][100][other]).all()
    st = steps(case)[0]
    for qi in range(case.Q):
        b = np.sort(s[qi, rows])
        assert np.diff(b).min() > 4 * tol, "band scores of query %d: %.3e apart, 4 tol = %.3e" % (qi, np.diff(b).min(), 4 * tol)
        qn = float(np.linalg.norm(I["q"][qi].astype(np.float64)))
        assert b[-1] - b[0] < _eps32(case) * qn, "the band is wider than the fp32 bound"
        after = after_mask(case, st)[qi, rows]
        assert int(after.sum()) == BAND // 2                      # the cursor stands in the middle of them ...
        wi = expected(case, st)[1][qi] - case.id_base
        assert np.isin(rows[after], wi).all() and not np.isin(rows[~after], wi).any()   # ... and the answer holds one half whole


def _overflow_preconditions(case, st):
    """a buffer takes SSE_COLLECT_CAP rows; only the planted queries of a step that claims it may overflow"""
    I = inputs(case)
    s, group = I["s"], I["group"]
    if not st.brute:
        # A query collects tag-eligible rows from its threshold up to the cursor's bracket.  With at most CAP eligible rows no
        # overflow is possible.  Larger indexes: the call runs at least 8 splits of 8 waves (k >= 1024 doubles the splits up
        # to 8; fewer queries than a chunk start there), so a maximum slot holds at most m rows, one per tile of its wave, the
        # k-th largest maximum is at least the (m k)-th best eligible score after the cursor, and threshold and bracket lie
        # within 4 e < 1e-4 of that and of the cursor.
        e = eligible(case)
        if e.sum(1).max() <= COLLECT_CAP:
            return
        nt = (case.N + 31) // 32
        m = -(-(-(-nt // 8)) // 8)
        assert 4 * _eps32(case) * scales(case)[0] < 1e-4
        ok = e & after_mask(case, st)
        for qi in range(case.Q):
            v = np.sort(s[qi][ok[qi]])[::-1]
            if v.size == 0:
                continue
            thr = v[min(m * st.k, v.size) - 1] - 1e-4
            assert int((e[qi] & (s[qi] >= thr) & (s[qi] <= v[0] + 1e-4)).sum()) <= COLLECT_CAP, (case.name, st.label, qi)
        return
    assert len(st.planted) == st.brute and case.base.ordinary_below and group.size > COLLECT_CAP and I["tags"] is None
    cur = cursors_of(case, st)
    for p in st.planted:
        # the copies are the strict maxima of the planted query (a unit row against itself), bit-equal in any arithmetic, and
        # the cursor score is theirs or +inf: no copy is below the bracket, so no copy takes part in the maxima, the threshold
        # lies under them and every copy is collected
        assert np.array_equal(order(case)[p, :group.size], group)
        assert cur[p][0] == "inf" or (cur[p][0] == "dev" and cur[p][1] < group.size)
    # another query never collects a copy: it scores them below zero, its cursor and so its threshold are positive -- a maximum
    # slot holds at most 4 rows of this index (188 tiles, 8 splits, 8 waves: 3 tiles per wave, one row of each per slot), so
    # the k-th largest maximum is at least the (4 k)-th best score after the cursor
    assert (case.N + 31) // 32 == 188
    ok = after_mask(case, st)
    for o_ in np.setdiff1d(np.arange(case.Q), st.planted):
        assert s[o_, group[0]] < 0
        v = np.sort(s[o_][ok[o_]])[::-1]
        assert v[4 * st.k - 1] > 1e-2
        assert case.N - group.size <= COLLECT_CAP


def check(case, step, scores, ids, counts):
    """The whole claim on one result.  Returns the worst |score - reference| over the real entries."""
    ws, wi, wc = expected(case, step)
    scores, ids, counts = np.asarray(scores), np.asarray(ids), np.asarray(counts)
    assert scores.shape == ws.shape and ids.shape == wi.shape and counts.shape == wc.shape, (scores.shape, ids.shape, counts.shape)
    assert scores.dtype == np.float64 and ids.dtype == np.int64 and counts.dtype == np.int32
    tag = "%s %s" % (case.name, step.label)
    assert np.array_equal(counts, wc), "%s: counts %s, want %s" % (tag, counts.tolist()[:16], wc.tolist()[:16])
    real = np.arange(step.k)[None, :] < wc[:, None]
    assert (ids[~real] == PAD_ID).all() and np.array_equal(scores[~real], np.full(int((~real).sum()), -np.inf)), \
        "%s: a padding slot holds something else than (-inf, INT64_MAX)" % tag
    rows = ids - case.id_base
    inside = (rows >= 0) & (rows < case.N)
    assert inside[real].all(), "%s: a row id outside the index" % tag
    qq = np.broadcast_to(np.arange(case.Q)[:, None], ids.shape)
    assert eligible(case)[qq[real], rows[real]].all(), "%s: an ineligible id in a result" % tag
    assert after_mask(case, step)[qq[real], rows[real]].all(), "%s: a row that is not after the cursor" % tag
    bad = np.argwhere(ids != wi)
    assert bad.size == 0, "%s: %d ids differ, first at query %d rank %d: got %d, want %d" % (
        tag, len(bad), bad[0][0], bad[0][1], ids[tuple(bad[0])], wi[tuple(bad[0])])
    assert not np.isnan(scores).any()
    worst = float(np.abs(scores[real] - ws[real]).max()) if real.any() else 0.0
    assert worst <= score_bar(case), "%s: score off by %.3e, bar %.3e" % (tag, worst, score_bar(case))
    for qi in range(case.Q):
        c = int(wc[qi])
        assert len(set(ids[qi, :c].tolist())) == c, "%s: a row id twice in one list" % tag
        if c < 2:
            continue
        d = scores[qi, 1:c] - scores[qi, :c - 1]
        assert (d <= 0).all(), "%s: scores increase along a list" % tag
        assert (ids[qi, 1:c] > ids[qi, :c - 1])[d == 0].all(), "%s: an exact tie with the higher row first" % tag
    return worst


# ---- the contract once more in numpy: what the layers above the library are tested on without a GPU

def after_on_host(full_s, full_i, k, after=None, ok=None):
    """The contract applied to whole ranked lists: full_s / full_i [Q, N] in score_topk's order, after = (scores, ids) or None,
    ok [Q, N] bool = eligibility of the entries (None: all).  IEEE comparisons on the scores given."""
    Q = full_s.shape[0]
    ws = np.full((Q, k), -np.inf)
    wi = np.full((Q, k), PAD_ID, np.int64)
    wc = np.zeros(Q, np.int32)
    for qi in range(Q):
        keep = np.ones(full_s.shape[1], bool) if ok is None else ok[qi].copy()
        if after is not None:
            with np.errstate(invalid="ignore"):
                keep &= (full_s[qi] < after[0][qi]) | ((full_s[qi] == after[0][qi]) & (full_i[qi] > after[1][qi]))
        c = min(k, int(keep.sum()))
        ws[qi, :c], wi[qi, :c], wc[qi] = full_s[qi, keep][:c], full_i[qi, keep][:c], c
    return ws, wi, wc


class OracleHandle:
    """Handle.score_topk and Handle.score_topk_after on the float64 oracle (numpy arrays in and out)."""

    def __init__(self, t, id_base=0, tags=None):
        self.t, self.id_base, self.tags = np.asarray(t, np.float64), int(id_base), tags
        self.calls = 0

    def _full(self, q):
        s = O.scores_f64(np.asarray(q, np.float32), self.t)
        o = np.argsort(-s, axis=1, kind="stable")
        return np.take_along_axis(s, o, 1), o.astype(np.int64) + self.id_base, o

    def score_topk(self, q, k):
        fs, fi, _ = self._full(q)
        return np.ascontiguousarray(fs[:, :k]), np.ascontiguousarray(fi[:, :k])

    def score_topk_after(self, q, k, after=None, any_of=None, none_of=None):
        self.calls += 1
        if not 1 <= k <= 1024:
            raise ValueError("k")
        fs, fi, o = self._full(q)
        ok = None
        if any_of is not None or none_of is not None:
            assert self.tags is not None
            tg = self.tags[o]
            ok = np.ones(o.shape, bool)
            if any_of is not None:
                a = np.asarray(any_of, np.uint64)[:, None]
                ok &= (a == 0) | ((tg & a) != 0)
            if none_of is not None:
                ok &= (tg & np.asarray(none_of, np.uint64)[:, None]) == 0
        return after_on_host(fs, fi, k, after, ok)
