"""Cases shared by tests/test_gpu_score_filtered.py (GPU) and tests/test_filtered_cases_host.py (CPU): sse_score_topk_filtered,
the exact top-k among the rows a query may return (tag masks any_of / none_of, excluded ids).  DESIGN K6g.

One list, CASES.  Per case: inputs(case) builds queries, index, tags, masks and exclusion lists from the case's seed (the index
and queries are those of a tests/topk_cases.py case: its constructions of copies and planted queries are reused), eligible(case)
is the [Q, N] truth table of the filter, expected(case) the float64 reference -- O.scores_f64, the ineligible columns removed,
O.topk, (-inf, INT64_MAX) padding, counts -- preconditions(case) proves the reference is one the device can be held to, and
check(case, scores, ids, counts) is what every entry point's result must pass.  The counter deltas a call must cause:

  score_filtered_bruteforce_queries   +1 per query whose collect buffer (SSE_COLLECT_CAP = 4096 rows) overflowed: `brute`, exact
  score_filtered_collected_rows       every row of the answer was re-scored by the select stage: at least the sum of the
                                      counts of the queries the float64 sweep did not take (`collected_min`)
  score_filtered_tiles_skipped        > 0, or exactly 0, where the case's variant says so (`skipped`)

No GPU import here."""
import functools

import numpy as np

from oracle import sse_oracle as O
from tests import topk_cases as TC
from tests.rank_cases import quarter_set  # noqa: F401  (the exact-in-any-order construction, used by the two-rank test)
from tests.topk_cases import BASE, unit  # noqa: F401

COLLECT_CAP = TC.COLLECT_CAP
PAD_ID = np.iinfo(np.int64).max
U1 = np.uint64(1)


def bit(b):
    return U1 << np.uint64(b)


class Case:
    def __init__(self, name, base, k, build, brute=0, counts=None, same_as_topk=False, variants=None, tag_entry="host", why=""):
        self.name, self.base, self.k, self.build = name, base, k, build
        self.Q, self.N, self.S, self.id_base, self.upload = base.Q, base.N, base.S, base.id_base, base.upload
        self.brute = brute                # delta of score_filtered_bruteforce_queries per call
        self.counts = counts              # the counts the case claims (None: whatever the reference says, all == k unless short)
        self.same_as_topk = same_as_topk  # the GPU test also compares with Handle.score_topk of the same handle
        # (label, score_filtered_skip, "any" | "none": how the tag requirement is handed over, skipped: "pos" | 0 | None)
        self.variants = variants or (("default", 1, "any", None),)
        self.tag_entry = tag_entry        # host: index_set_tags | dev: index_set_tags_dev
        self.why = why

    def __repr__(self):
        return self.name


def _base(name, Q, N, S, k, **kw):
    return TC.Case(name, Q, N, S, min(k, N), seed=kw.pop("seed", 7000 + Q + N + S + k), **kw)


# ---- builders: (case, q, t, group, s, rng) -> dict(tags, any, none, exclude); q / t may be edited in place before freezing

def _b_none(case, q, t, group, s, rng):
    return {}


def _b_one_of(nbits, two=False):
    def build(case, q, t, group, s, rng):
        tags = (U1 << rng.randint(0, nbits, size=case.N).astype(np.uint64)).astype(np.uint64)
        any_ = (U1 << rng.randint(0, nbits, size=case.Q).astype(np.uint64)).astype(np.uint64)
        if two:
            any_ |= (U1 << rng.randint(0, nbits, size=case.Q).astype(np.uint64)).astype(np.uint64)
        return dict(tags=tags, any=any_)
    return build


def _b_best_ineligible(case, q, t, group, s, rng):
    tags = np.zeros(case.N, np.uint64)
    order = np.argsort(-s, axis=1, kind="stable")
    for qi in range(case.Q):
        tags[order[qi, :100]] |= bit(qi)
    return dict(tags=tags, none=np.array([bit(qi) for qi in range(case.Q)], np.uint64))


def _b_fewer(case, q, t, group, s, rng):
    tags = np.full(case.N, bit(3), np.uint64)
    tags[[7, 250, 499]] = bit(0)          # first tile, middle, the last row (tail tile: 500 = 15 * 32 + 20)
    tags[333] = bit(1)
    return dict(tags=tags, any=np.array([bit(0), bit(1), bit(2), bit(3)], np.uint64))


def _b_tail(case, q, t, group, s, rng):
    q[0] = t[case.N - 1]                   # a unit row against itself: the strict maximum of query 0
    tags = (U1 << (np.arange(case.N) % 2).astype(np.uint64)).astype(np.uint64)
    tags[case.N - 1] = bit(0)
    return dict(tags=tags, any=np.array([bit(0), bit(1)], np.uint64))


def _b_half(case, q, t, group, s, rng):
    tags = (U1 << rng.randint(0, 2, size=case.N).astype(np.uint64)).astype(np.uint64)
    return dict(tags=tags, any=np.full(case.Q, bit(0), np.uint64))


def _b_tie(case, q, t, group, s, rng):
    tags = np.full(case.N, bit(0), np.uint64)
    tags[group[1::2]] = bit(1)             # every second copy is ineligible
    return dict(tags=tags, any=np.full(case.Q, bit(0), np.uint64))


def _b_overflow(case, q, t, group, s, rng):
    tags = (U1 << rng.randint(0, 2, size=case.N).astype(np.uint64)).astype(np.uint64)
    tags[group] = bit(0)                   # all 4500 copies eligible
    return dict(tags=tags, any=np.full(case.Q, bit(0), np.uint64))


def _b_excl3(case, q, t, group, s, rng):
    order = np.argsort(-s, axis=1, kind="stable")
    return dict(exclude=np.ascontiguousarray(order[:, :3].astype(np.int64) + case.id_base))


def _b_excl64(case, q, t, group, s, rng):
    tags = (U1 << rng.randint(0, 2, size=case.N).astype(np.uint64)).astype(np.uint64)
    order = np.argsort(-s, axis=1, kind="stable")
    ex = np.full((case.Q, 64), -1, np.int64)                  # -1 padding
    for qi in range(case.Q):
        el = [r for r in order[qi, :60] if tags[r] == bit(0)]
        inel = [r for r in order[qi, :60] if tags[r] != bit(0)]
        ex[qi, 0:5] = el[:5]                                  # the five best eligible rows ...
        ex[qi, 5:10] = el[:5]                                 # ... twice
        ex[qi, 10:14] = el[6:10]                              # (the sixth best stays)
        ex[qi, 14:20] = inel[:6]                              # rows the tags already removed
        ex[qi, 20:24] = [case.N, case.N + 5, 2 ** 40, -case.N]  # outside the index
        ex[qi, 40:44] = el[10:14]
    return dict(tags=tags, any=np.full(case.Q, bit(0), np.uint64), exclude=ex + np.where(ex == -1, 0, case.id_base))


def _b_shard(case, q, t, group, s, rng):
    tags = (U1 << rng.randint(0, 4, size=case.N).astype(np.uint64)).astype(np.uint64)
    any_ = np.array([bit(qi % 4) | bit((qi + 1) % 4) for qi in range(case.Q)], np.uint64)
    order = np.argsort(-s, axis=1, kind="stable")
    ex = order[:, :2].astype(np.int64) + case.id_base         # global ids
    ex = np.concatenate([ex, order[:, :1].astype(np.int64)], axis=1)   # the best row's LOCAL number: not an id of this shard
    return dict(tags=tags, any=any_, none=np.full(case.Q, bit(9), np.uint64), exclude=np.ascontiguousarray(ex))


def _b_sorted(case, q, t, group, s, rng):
    tags = (U1 << (np.arange(case.N) // 512).astype(np.uint64)).astype(np.uint64)    # 8 groups of 512 rows = 16 tiles each
    any_ = np.full(case.Q, bit(0), np.uint64)
    any_[32:] = (U1 << rng.randint(0, 2, size=case.Q - 32).astype(np.uint64)).astype(np.uint64)   # tags 0 and 1 only
    return dict(tags=tags, any=any_)


def _b_sixteen_blocks(case, q, t, group, s, rng):
    per = (case.N + 15) // 16                                # 16 runs of rows, a tag each; a query takes runs b and b + 8
    tags = (U1 << (np.arange(case.N) // per).astype(np.uint64)).astype(np.uint64)
    return dict(tags=tags, any=np.array([bit(qi % 8) | bit(qi % 8 + 8) for qi in range(case.Q)], np.uint64))


CASES = [
    Case("no_filter_k10", _base("nf", 5, 3000, 32, 10, seed=7101), 10, _b_none, same_as_topk=True, why="score_topk's bits, k <= 16"),
    Case("no_filter_k40", _base("nf", 5, 3000, 32, 40, seed=7101), 40, _b_none, same_as_topk=True, why="score_topk's bits, k > 16"),
    Case("one_of_eight", _base("o8", 5, 3000, 32, 10), 10, _b_one_of(8), why="the plain route"),
    Case("best_rows_ineligible", _base("bi", 9, 2000, 32, 20), 20, _b_best_ineligible, why="threshold from eligible rows only"),
    Case("fewer_than_k", _base("fk", 4, 500, 16, 10), 10, _b_fewer, counts=(3, 1, 0, 10), why="counts 3, 1, 0; padding; theta = -inf"),
    Case("tail_tile_k33", _base("tt", 2, 33, 5, 33, seed=7105), 33, _b_tail, counts=(17, 16), why="tail masking, S < 8, k = N"),
    Case("tail_tile_k40", _base("tt", 2, 33, 5, 40, seed=7105), 40, _b_tail, counts=(17, 16), why="k > N"),
    Case("q33_nq4_partial_tile", _base("n4", 33, 2000, 64, 40), 40, _b_one_of(4, two=True), why="NQ = 4, partial second query tile"),
    Case("s300_nq2", _base("n2", 40, 700, 300, 40), 40, _b_one_of(4, two=True), why="NQ = 2"),
    Case("s620_nq1", _base("n1", 40, 700, 620, 40), 40, _b_one_of(4, two=True), why="NQ = 1 with Q > 32"),
    Case("k1024_half_eligible", _base("k1", 3, 5000, 64, 1024), 1024, _b_half, why="largest k: threshold from enough maxima"),
    Case("tie_inside_k", TC.Case("ft", 9, 2000, 32, 20, kind="tie", seed=11, copies=30, planted=(4,)), 20, _b_tie,
         why="tie order by id among the eligible copies only"),
    Case("overflow", TC.Case("fo", 8, 6000, 64, 50, kind="dup", seed=14, copies=4500, planted=(3,), ordinary_below=True), 50,
         _b_overflow, brute=1, why="4500 eligible copies > 4096: the float64 sweep serves the planted query alone"),
    Case("exclude_3_best", _base("e3", 6, 3000, 32, 10, seed=7110), 10, _b_excl3, why="exclusion in threshold and select"),
    Case("exclude_64_mixed", _base("e6", 6, 3000, 32, 10, seed=7110), 10, _b_excl64,
         why="duplicates, ids outside the index, -1 padding, ids the tags already removed"),
    Case("shard_base_dev", _base("sb", 9, 1200, 40, 33, seed=7111, upload="dev", id_base=BASE), 33, _b_shard, tag_entry="dev",
         why="index_set_dev + index_set_tags_dev: ids global, exclusion by global id"),
    Case("shard_base_f64", _base("sb", 9, 1200, 40, 33, seed=7111, upload="f64", id_base=BASE), 33, _b_shard,
         why="float64 index: idx64 branch of wave_exact_dot"),
    Case("sorted_tags", _base("st", 64, 4096, 32, 10), 10, _b_sorted,
         variants=(("skip_on", 1, "any", "pos"), ("skip_off", 0, "any", 0), ("any_null", 1, "none", 0)),
         why="rows grouped by tag: tiles of tags 2 .. 7 skipped; results equal with the option off and with none_of in place of any_of"),
    Case("folded_splits", _base("fs", 5, 16400, 16, 10), 10, _b_sixteen_blocks, variants=(("skip_on", 1, "any", "pos"),),
         why="513 tiles, 5 queries: 32 index splits share 16 x 256 maxima slots (atomicMax), eligible rows on both sides of a fold"),
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(q, t, group, tags, any, none, exclude): arrays or None, read-only."""
    q0, t0, group = TC.inputs(case.base)
    q, t = q0.copy(), t0.copy()
    rng = np.random.RandomState(case.base.seed + 99)
    if case.build is _b_tail:
        _b_tail(case, q, t, group, None, np.random.RandomState(0))      # (edits q before the scores are formed)
    s = _scores(case, q, t, group)
    d = dict(tags=None, any=None, none=None, exclude=None)
    d.update(case.build(case, q, t, group, s, rng))
    d.update(q=q, t=t, group=group, s=s)
    for v in d.values():
        if v is not None:
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


def masks(case, form="any"):
    """(any_of, none_of) as handed to the call.  form "none": the same requirement expressed by none_of alone (one-hot tags:
    'a bit of any_of' == 'no bit of the other tags in use')."""
    I = inputs(case)
    if form == "any":
        return I["any"], I["none"]
    assert I["none"] is None and I["any"] is not None
    used = np.bitwise_or.reduce(I["tags"])
    assert ((I["tags"] & (I["tags"] - U1)) == 0).all() and (I["tags"] != 0).all(), "one-hot tags"
    return None, (used & ~I["any"]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def eligible(case, form="any"):
    I = inputs(case)
    any_, none_ = masks(case, form)
    e = np.ones((case.Q, case.N), bool)
    if I["tags"] is not None:
        tg = I["tags"][None, :]
        if any_ is not None:
            e &= (any_[:, None] == 0) | ((tg & any_[:, None]) != 0)
        if none_ is not None:
            e &= (tg & none_[:, None]) == 0
    if I["exclude"] is not None:
        for qi in range(case.Q):
            r = I["exclude"][qi] - case.id_base
            e[qi, r[(r >= 0) & (r < case.N)]] = False
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def reference(case, k=None):
    """(scores float64 [Q,k], ids int64 [Q,k], counts int32 [Q]), read-only."""
    k = case.k if k is None else k
    s, e = inputs(case)["s"], eligible(case)
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
    return ws, wi, cnt


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
    """every answer row of a query the float64 sweep did not take was re-scored by the select stage"""
    cnt = reference(case)[2].astype(np.int64)
    if case.brute:
        cnt = np.delete(cnt, list(case.base.planted))
    return int(cnt.sum())


def preconditions(case):
    """AssertionError unless the reference is one a device summing in its own order must reproduce id for id, and every count
    and every overflow is the one the case claims."""
    I = inputs(case)
    q, t, group, s = I["q"], I["t"], I["group"], I["s"]
    tol = scales(case)[2]
    e = eligible(case)
    assert q.shape == (case.Q, case.S) and t.shape == (case.N, case.S) and 1 <= case.k <= 1024
    assert I["exclude"] is None or I["exclude"].shape[1] <= 64
    in_group = np.zeros(case.N, bool)
    if group.size:
        tb = np.ascontiguousarray(t[group])
        assert (tb.view(np.uint8) == tb[:1].view(np.uint8)).all(), "copies are not bit-equal rows"
        assert len({t[r].tobytes() for r in range(case.N)}) == case.N - group.size + 1, "an unplanned duplicate row"
        in_group[group] = True
    ws, wi, cnt = reference(case, min(case.k + 1, 1 << 20))
    for qi in range(case.Q):
        c = int(cnt[qi])
        if c < 2:
            continue
        rows = wi[qi, :c] - case.id_base
        gap = ws[qi, :c - 1] - ws[qi, 1:c]
        both = in_group[rows[:-1]] & in_group[rows[1:]]
        assert (gap[both] == 0).all()
        if (~both).any():
            assert gap[~both].min() > 2 * tol, "%s query %d: neighbours %.3e apart, 2 tol = %.3e" % (case.name, qi, gap[~both].min(), 2 * tol)
    want_counts = np.minimum(e.sum(1), case.k)
    assert np.array_equal(reference(case)[2], want_counts)
    if case.counts is not None:
        assert tuple(int(c) for c in want_counts) == tuple(case.counts), (case.name, want_counts)
    elif case.N >= case.k + 200:
        assert (want_counts == case.k).all(), (case.name, want_counts)
    # overflow: a buffer takes SSE_COLLECT_CAP rows and holds tag-eligible rows only
    tag_e = eligible_by_tags(case)
    if case.brute == 0:
        assert tag_e.sum(1).max() <= COLLECT_CAP, "%s: an overflow the case does not claim is possible" % case.name
    else:
        planted = list(case.base.planted)
        assert len(planted) == case.brute and case.base.ordinary_below
        for p in planted:
            # the eligible copies are the strict maxima of their own row (Cauchy-Schwarz), bit-equal in any arithmetic: all
            # of them are at or above any threshold that keeps k rows
            assert (tag_e[p, group]).all() and group.size > COLLECT_CAP and np.array_equal(wi[p, :case.k] - case.id_base, group[:case.k])
        others = np.setdiff1d(np.arange(case.Q), planted)
        # another query never collects a copy: it scores them below zero, and its threshold is positive -- a maximum slot of
        # the sweep holds at most 4 rows of this index (188 tiles, 8 splits, 8 waves: 3 tiles per wave, one row of each per
        # slot), so the (k + n_excl)-th largest maximum is at least the 4 (k + n_excl)-th best eligible score, far above
        # twice the fp32 bound 2 (S + 2) 5.97e-8
        assert (case.N + 31) // 32 == 188 and I["exclude"] is None
        for o in others:
            assert s[o, group[0]] < 0
            best = np.sort(s[o][tag_e[o]])[::-1]
            assert best[4 * case.k - 1] > 1e-2
            assert int((tag_e[o] & ~in_group).sum()) <= COLLECT_CAP
    for label, _opt, form, _sk in case.variants:
        assert np.array_equal(eligible(case, form), e), label
    return True


def eligible_by_tags(case):
    """the truth table without the exclusion lists (what a sweep can collect)"""
    I = inputs(case)
    e = np.ones((case.Q, case.N), bool)
    if I["tags"] is not None:
        tg = I["tags"][None, :]
        if I["any"] is not None:
            e &= (I["any"][:, None] == 0) | ((tg & I["any"][:, None]) != 0)
        if I["none"] is not None:
            e &= (tg & I["none"][:, None]) == 0
    return e


def check(case, scores, ids, counts):
    """The whole claim on one result.  Returns the worst |score - reference| over the real entries."""
    ws, wi, wc = expected(case)
    scores, ids, counts = np.asarray(scores), np.asarray(ids), np.asarray(counts)
    assert scores.shape == ws.shape and ids.shape == wi.shape and counts.shape == wc.shape, (scores.shape, ids.shape, counts.shape)
    assert scores.dtype == np.float64 and ids.dtype == np.int64 and counts.dtype == np.int32
    assert np.array_equal(counts, wc), "%s: counts %s, want %s" % (case.name, counts.tolist()[:16], wc.tolist()[:16])
    real = np.arange(case.k)[None, :] < wc[:, None]
    assert (ids[~real] == PAD_ID).all() and np.array_equal(scores[~real], np.full(int((~real).sum()), -np.inf)), \
        "%s: a padding slot holds something else than (-inf, INT64_MAX)" % case.name
    e = eligible(case)
    rows = ids - case.id_base
    inside = (rows >= 0) & (rows < case.N)
    assert inside[real].all(), "%s: a row id outside the index" % case.name
    qq = np.broadcast_to(np.arange(case.Q)[:, None], ids.shape)
    assert e[qq[real], rows[real]].all(), "%s: an ineligible id in a result" % case.name
    bad = np.argwhere(ids != wi)
    assert bad.size == 0, "%s: %d ids differ, first at query %d rank %d: got %d, want %d" % (
        case.name, len(bad), bad[0][0], bad[0][1], ids[tuple(bad[0])], wi[tuple(bad[0])])
    assert not np.isnan(scores).any()
    worst = float(np.abs(scores[real] - ws[real]).max()) if real.any() else 0.0
    assert worst <= score_bar(case), "%s: score off by %.3e, bar %.3e" % (case.name, worst, score_bar(case))
    for qi in range(case.Q):
        c = int(wc[qi])
        assert len(set(ids[qi, :c].tolist())) == c, "%s: a row id twice in one list" % case.name
        if c < 2:
            continue
        d =scores[qi, 1:c] - scores[qi, :c - 1]
        assert (d <= 0).all(), "%s: scores increase along a list" % case.name
        assert (ids[qi, 1:c] > ids[qi, :c - 1])[d == 0].all(), "%s: an exact tie with the higher row first" % case.name
    return worst
