"""Cases shared by tests/test_gpu_score_grouped.py (GPU) and tests/test_grouped_cases_host.py (CPU): sse_score_topk_grouped, the
exact top-k DISTINCT groups of index rows (int64 group keys per row, tag masks any_of / none_of).  DESIGN K6h.

One list, CASES.  Per case: inputs(case) builds queries, index, group keys, tags and masks from the case's seed (the index and
queries are those of a tests/topk_cases.py case: its constructions of copies and planted queries are reused), eligible(case) is
the [Q, N] truth table of the tag rule, reference(case) the float64 reference -- O.scores_f64 (one score per set of bit-equal
rows), the full ranking of the eligible columns by O.topk, every row whose group already appeared to its left removed, cut to
k, (-inf, INT64_MAX, INT64_MAX) padding, counts -- preconditions(case) proves the reference is one the device can be held to,
and check(case, scores, ids, groups, counts) is what every entry point's result must pass.  The counter deltas of a call:

  score_grouped_bruteforce_queries   +1 per query whose collect buffer (SSE_COLLECT_CAP = 4096 rows) overflowed.  Proven per
                                     query (brute_class): "no" -- at most 4096 tag-eligible rows in total, nothing can overflow;
                                     "yes" -- more than 4096 eligible bit-equal copies that are the query's strict maxima (all
                                     of them are at or above any threshold), or fewer than k groups among more than 4096
                                     eligible rows (theta = -inf: everything eligible is collected); otherwise "unknown", and
                                     a case with such a query leaves the counter unchecked (brute = -1)
  score_grouped_collected_rows       every answer entry of a "no" query was re-scored by the select stage: at least the sum of
                                     their counts (`collected_min`)

No GPU import here."""
import functools

import numpy as np

from oracle import sse_oracle as O
from tests import topk_cases as TC
from tests.filtered_cases import U1, _b_sixteen_blocks, bit
from tests.topk_cases import BASE, unit  # noqa: F401

COLLECT_CAP = TC.COLLECT_CAP
PAD = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min


class Case:
    def __init__(self, name, base, k, build, brute=0, counts=None, same_as_topk=False, group_entry="host", prep=None, why=""):
        self.name, self.base, self.k, self.build = name, base, k, build
        self.Q, self.N, self.S, self.id_base, self.upload = base.Q, base.N, base.S, base.id_base, base.upload
        self.brute = brute                # delta of score_grouped_bruteforce_queries per call; -1: not derived
        self.counts = counts              # the counts the case claims (None: all == k)
        self.same_as_topk = same_as_topk  # the GPU test also compares scores and ids with Handle.score_topk of the same handle
        self.group_entry = group_entry    # host: index_set_groups / index_set_tags | dev: the _dev forms
        self.prep = prep                  # (q, t) edited in place before the scores are formed
        self.why = why

    def __repr__(self):
        return self.name


def _base(name, Q, N, S, k, **kw):
    return TC.Case(name, Q, N, S, min(k, N), seed=kw.pop("seed", 8000 + Q + N + S + k), **kw)


def _spread(n, rng):
    """n distinct keys in random order over the whole int64 range: negatives, values above 2^40, both ends"""
    keys = np.unique(np.concatenate([rng.randint(-2 ** 62, 2 ** 62, size=n + 16).astype(np.int64) * 2,
                                     np.array([I64_MIN, PAD, -1, 0, 1, 2 ** 40 + 5, -(2 ** 40) - 5, 2 ** 32], np.int64)]))
    assert keys.size >= n
    special = np.array([I64_MIN, PAD, -1, 0, 2 ** 40 + 5], np.int64)
    rest = np.setdiff1d(keys, special)
    keys = np.concatenate([special, rng.permutation(rest)])[:n]
    return rng.permutation(keys)


# ---- builders: (case, q, t, copies, s, rng) -> dict(groups, tags, any, none)

def _b_own(case, q, t, copies, s, rng):
    return dict(groups=_spread(case.N, rng))


def _b_random(per):
    def build(case, q, t, copies, s, rng):
        pool = _spread(max(case.N // per, 1), rng)
        g = pool[rng.randint(0, pool.size, size=case.N)]
        g[:pool.size] = pool                                   # every key in use, the special ones among them
        return dict(groups=g)
    return build


def _b_exact(per):
    def build(case, q, t, copies, s, rng):
        pool = _spread((case.N + per - 1) // per, rng)
        return dict(groups=pool[rng.permutation(case.N) // per])
    return build


def _b_best100(case, q, t, copies, s, rng):
    g = _spread(case.N, rng)
    order = np.argsort(-s, axis=1, kind="stable")
    g[np.unique(order[:, :100])] = 77                          # the best 100 rows of every query: one group
    return dict(groups=g)


def _b_one_group(case, q, t, copies, s, rng):
    return dict(groups=np.full(case.N, -5, np.int64))


def _b_three(case, q, t, copies, s, rng):
    return dict(groups=np.array([I64_MIN, 3, PAD], np.int64)[rng.randint(0, 3, size=case.N)])


def _prep_tail(q, t):
    q[0] = t[t.shape[0] - 1]                                   # a unit row against itself: the strict maximum of query 0


def _b_pairs(case, q, t, copies, s, rng):
    return dict(groups=(np.arange(case.N, dtype=np.int64) // 2) * 1000 - 7000)


def _b_tags4(per):
    def build(case, q, t, copies, s, rng):
        d = _b_random(per)(case, q, t, copies, s, rng)
        d["tags"] = (U1 << rng.randint(0, 4, size=case.N).astype(np.uint64)).astype(np.uint64)
        d["any"] = ((U1 << rng.randint(0, 4, size=case.Q).astype(np.uint64)) | (U1 << rng.randint(0, 4, size=case.Q).astype(np.uint64))).astype(np.uint64)
        return d
    return build


def _b_tie_three(case, q, t, copies, s, rng):
    g = _spread(case.N, rng)
    g[copies] = np.array([900, -900, 2 ** 41], np.int64)[np.arange(copies.size) % 3]
    return dict(groups=g)


def _b_tie_one(case, q, t, copies, s, rng):
    g = _spread(case.N, rng)
    g[copies] = 900
    return dict(groups=g)


def _b_dup(case, q, t, copies, s, rng):
    g = _spread(case.N, rng)
    g[copies] = 424242
    tags = np.full(case.N, bit(0) | bit(1), np.uint64)
    tags[copies] = bit(0)                                      # the copies: for the planted query alone
    any_ = np.full(case.Q, bit(1), np.uint64)
    any_[list(case.base.planted)] = bit(0)
    return dict(groups=g, tags=tags, any=any_)


def _b_masks(case, q, t, copies, s, rng):
    d = _b_exact(8)(case, q, t, copies, s, rng)
    g = d["groups"].copy()
    tags = np.zeros(case.N, np.uint64)
    order = np.argsort(-s, axis=1, kind="stable")
    for qi in range(case.Q):                                   # the next group's second row: the query's next best row
        best = g[order[qi, 0]]
        nxt, mate = [r for r in order[qi, :40] if g[r] != best][:2]
        g[mate] = g[nxt]
    d["groups"] = g
    for qi in range(case.Q):
        best = g[order[qi, 0]]
        tags[g == best] |= bit(qi)                             # the best group: every row ineligible
        nxt = next(r for r in order[qi] if g[r] != best)
        tags[nxt] |= bit(qi)                                   # the next group: its best row ineligible, its second row stays
    d.update(tags=tags, none=np.array([bit(qi) for qi in range(case.Q)], np.uint64))
    return d


def _b_shard(case, q, t, copies, s, rng):
    d = _b_random(5)(case, q, t, copies, s, rng)
    d["tags"] = (U1 << rng.randint(0, 4, size=case.N).astype(np.uint64)).astype(np.uint64)
    d["any"] = np.array([bit(qi % 4) | bit((qi + 1) % 4) for qi in range(case.Q)], np.uint64)
    d["none"] = np.full(case.Q, bit(9), np.uint64)
    return d


def _b_folded(case, q, t, copies, s, rng):
    d = _b_random(8)(case, q, t, copies, s, rng)
    d.update(_b_sixteen_blocks(case, q, t, copies, s, rng))    # rows in 16 runs by tag: whole tiles without an eligible row
    return d


CASES = [
    Case("own_group_k10", _base("og", 5, 3000, 32, 10, seed=8101), 10, _b_own, same_as_topk=True, why="score_topk's bits, k <= 16"),
    Case("own_group_k40", _base("og", 5, 3000, 32, 40, seed=8101), 40, _b_own, same_as_topk=True, why="score_topk's bits, k > 16"),
    Case("random_groups_of_8", _base("r8", 5, 3000, 32, 10), 10, _b_random(8), why="the plain route; keys over the whole int64 range"),
    Case("best_100_in_one_group", _base("b1", 9, 2000, 32, 20), 20, _b_best100,
         why="the k-th MAXIMUM is inside the first group: a threshold from it returns short counts"),
    Case("one_group", _base("g1", 4, 500, 16, 10), 10, _b_one_group, counts=(1, 1, 1, 1), why="count 1"),
    Case("three_groups", _base("g3", 4, 500, 16, 10), 10, _b_three, counts=(3, 3, 3, 3), why="fewer groups than k: theta = -inf, everything collected"),
    Case("three_groups_n5000", _base("g3", 4, 5000, 16, 10), 10, _b_three, counts=(3, 3, 3, 3), brute=4,
         why="everything collected overflows: the float64 sweep's group reduction with LDS refills"),
    Case("tail_tile_k33", _base("tt", 2, 33, 5, 33, seed=8105), 33, _b_pairs, counts=(17, 17), prep=_prep_tail, why="tail masking, S < 8, k = N"),
    Case("tail_tile_k40", _base("tt", 2, 33, 5, 40, seed=8105), 40, _b_pairs, counts=(17, 17), prep=_prep_tail, why="k > N"),
    Case("q33_nq4_partial_tile", _base("n4", 33, 2000, 64, 40), 40, _b_tags4(4), why="collect at NQ = 4, partial second query tile"),
    Case("s300_nq2", _base("n2", 40, 700, 300, 40), 40, _b_tags4(3), why="NQ = 2"),
    Case("s620_nq1", _base("n1", 40, 700, 620, 40), 40, _b_tags4(3), why="NQ = 1 with Q > 32"),
    Case("k1024_groups_of_2", _base("k1", 3, 4000, 64, 1024), 1024, _b_exact(2), why="largest k: 2000 groups"),
    Case("tie_over_three_groups", TC.Case("gt", 9, 2000, 32, 20, kind="tie", seed=11, copies=30, planted=(4,)), 20, _b_tie_three,
         why="equal group scores order by representative id; each representative its group's lowest copy"),
    Case("tie_in_one_group", TC.Case("gt", 9, 2000, 32, 20, kind="tie", seed=11, copies=30, planted=(4,)), 20, _b_tie_one,
         why="30 equal rows, one entry"),
    Case("overflow_in_one_group", TC.Case("go", 8, 6000, 64, 50, kind="dup", seed=14, copies=4500, planted=(3,), ordinary_below=True), 50,
         _b_dup, brute=1, why="4500 eligible copies of one group > 4096: the float64 sweep serves the planted query alone"),
    Case("masks_remove_and_demote", _base("mk", 6, 3000, 32, 10), 10, _b_masks,
         why="the best group all ineligible: it vanishes; the next group is represented by its best ELIGIBLE row"),
    Case("shard_base_dev", _base("sb", 9, 1200, 40, 33, seed=8111, upload="dev", id_base=BASE), 33, _b_shard, group_entry="dev",
         why="index_set_dev + index_set_groups_dev + index_set_tags_dev: ids global"),
    Case("shard_base_f64", _base("sb", 9, 1200, 40, 33, seed=8111, upload="f64", id_base=BASE), 33, _b_shard,
         why="float64 index: idx64 branch of wave_exact_dot"),
    Case("folded_splits_skipped_tiles", _base("fs", 5, 16400, 16, 10), 10, _b_folded,
         why="513 tiles, 5 queries: 32 index splits share 16 x 256 (key, row) slots (64-bit atomicMax); tiles skipped in the max sweep"),
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(q, t, copies, s, groups, tags, any, none): arrays or None, read-only."""
    q0, t0, copies = TC.inputs(case.base)
    q, t = q0.copy(), t0.copy()
    if case.prep is not None:
        case.prep(q, t)
    s = _scores(case, q, t, copies)
    d = dict(tags=None, any=None, none=None)
    d.update(case.build(case, q, t, copies, s, np.random.RandomState(case.base.seed + 99)))
    d["groups"] = np.ascontiguousarray(d["groups"], dtype=np.int64)
    d.update(q=q, t=t, copies=copies, s=s)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def _scores(case, q, t, copies):
    """O.scores_f64; bit-equal rows get ONE reference score (the construction of topk_cases.reference_scores)."""
    t64 = np.asarray(t, np.float64)
    if copies.size:
        keep = np.ones(case.N, bool)
        keep[copies[1:]] = False
        col = np.cumsum(keep) - 1
        col[copies] = col[copies[0]]
        return np.ascontiguousarray(O.scores_f64(q, t64[keep])[:, col])
    return np.ascontiguousarray(O.scores_f64(q, t64))


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


@functools.lru_cache(maxsize=None)
def ranking(case):
    """per query: the eligible rows in the order of score_topk (score descending, equal scores by ascending row)"""
    s, e = inputs(case)["s"], eligible(case)
    out = []
    for qi in range(case.Q):
        cols = np.flatnonzero(e[qi])
        if cols.size:
            _, ii = O.topk(s[qi:qi + 1, cols], cols.size)
            cols = cols[ii[0]]
        out.append(cols)
    return out


def collapse(rows, groups):
    """the rows whose group did not appear to their left, in order"""
    _, first = np.unique(groups[rows], return_index=True)
    return rows[np.sort(first)]


@functools.lru_cache(maxsize=None)
def reference(case, k=None):
    """(scores float64 [Q,k], ids int64 [Q,k], groups int64 [Q,k], counts int32 [Q]), read-only."""
    k = case.k if k is None else k
    I = inputs(case)
    ws = np.full((case.Q, k), -np.inf)
    wi = np.full((case.Q, k), PAD, np.int64)
    wg = np.full((case.Q, k), PAD, np.int64)
    cnt = np.zeros(case.Q, np.int32)
    for qi, rows in enumerate(ranking(case)):
        reps = collapse(rows, I["groups"])[:k]
        c = reps.size
        cnt[qi] = c
        ws[qi, :c], wi[qi, :c], wg[qi, :c] = I["s"][qi, reps], reps + case.id_base, I["groups"][reps]
    for a in (ws, wi, wg, cnt):
        a.setflags(write=False)
    return ws, wi, wg, cnt


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


@functools.lru_cache(maxsize=None)
def brute_class(case):
    """per query "no" | "yes" | "unknown": what can be PROVEN about the float64 sweep (module docstring)"""
    I = inputs(case)
    e, copies, g, s = eligible(case), I["copies"], I["groups"], I["s"]
    out = []
    for qi in range(case.Q):
        rows = np.flatnonzero(e[qi])
        if rows.size <= COLLECT_CAP:
            out.append("no")
        elif np.unique(g[rows]).size < case.k:
            out.append("yes")                                  # theta = -inf: all rows.size > 4096 rows are collected
        elif copies.size and int(e[qi, copies].sum()) > COLLECT_CAP and s[qi, copies[0]] > np.delete(s[qi], copies).max():
            out.append("yes")                                  # more than 4096 bit-equal rows share the largest fp32 score
        else:
            out.append("unknown")
    return tuple(out)


def collected_min(case):
    """every answer entry of a query that certainly stays out of the float64 sweep was re-scored by the select stage"""
    cnt = reference(case)[3]
    return int(sum(int(c) for c, b in zip(cnt, brute_class(case)) if b == "no"))


def preconditions(case):
    """AssertionError unless the reference is one a device summing in its own order must reproduce id for id, and every count
    and every claimed overflow is certain."""
    I = inputs(case)
    q, t, copies, s, g = I["q"], I["t"], I["copies"], I["s"], I["groups"]
    tol = scales(case)[2]
    e = eligible(case)
    assert q.shape == (case.Q, case.S) and t.shape == (case.N, case.S) and g.shape == (case.N,) and g.dtype == np.int64
    assert 1 <= case.k <= 1024
    is_copy = np.zeros(case.N, bool)
    if copies.size:
        tb = np.ascontiguousarray(t[copies])
        assert (tb.view(np.uint8) == tb[:1].view(np.uint8)).all(), "copies are not bit-equal rows"
        assert len({t[r].tobytes() for r in range(case.N)}) == case.N - copies.size + 1, "an unplanned duplicate row"
        is_copy[copies] = True

    def apart(a, b, qi, what):
        """rows a, b of query qi: bit-equal rows with one score, or further apart than two summation orders can move them"""
        if is_copy[a] and is_copy[b]:
            assert s[qi, a] == s[qi, b]
        else:
            assert abs(s[qi, a] - s[qi, b]) > 2 * tol, "%s query %d %s: rows %d, %d are %.3e apart, 2 tol = %.3e" % (
                case.name, qi, what, a, b, abs(s[qi, a] - s[qi, b]), 2 * tol)

    want_counts = []
    for qi, rows in enumerate(ranking(case)):
        reps = collapse(rows, g)
        want_counts.append(min(case.k, reps.size))
        reps = reps[:case.k + 1]                               # the answer and the first group left out
        for a, b in zip(reps[:-1], reps[1:]):
            apart(a, b, qi, "neighbouring groups")
        # a representative and the runner-up of its own group: another summation order must not pick the other row
        answer = set(g[reps[:case.k]].tolist())
        seen = {}
        for r in rows:
            key = int(g[r])
            if key not in answer:
                continue
            seen.setdefault(key, []).append(r)
        for key, rr in seen.items():
            if len(rr) > 1:
                apart(rr[0], rr[1], qi, "inside group %d" % key)
    want_counts = np.array(want_counts, np.int32)
    assert np.array_equal(reference(case)[3], want_counts)
    assert np.array_equal(want_counts, np.minimum(case.k, [np.unique(g[e[qi]]).size for qi in range(case.Q)]))
    if case.counts is not None:
        assert tuple(int(c) for c in want_counts) == tuple(case.counts), (case.name, want_counts)
    else:
        assert (want_counts == case.k).all(), (case.name, want_counts)
    cls = brute_class(case)
    if case.brute == -1:
        assert "unknown" in cls, "%s: the counter could be claimed" % case.name
    else:
        assert "unknown" not in cls and cls.count("yes") == case.brute, (case.name, cls)
    return True


def check(case, scores, ids, groups, counts):
    """The whole claim on one result.  Returns the worst |score - reference| over the real entries."""
    ws, wi, wg, wc = expected(case)
    I = inputs(case)
    scores, ids, groups, counts = np.asarray(scores), np.asarray(ids), np.asarray(groups), np.asarray(counts)
    assert scores.shape == ws.shape and ids.shape == wi.shape and groups.shape == wg.shape and counts.shape == wc.shape, (
        scores.shape, ids.shape, groups.shape, counts.shape)
    assert scores.dtype == np.float64 and ids.dtype == np.int64 and groups.dtype == np.int64 and counts.dtype == np.int32
    assert np.array_equal(counts, wc), "%s: counts %s, want %s" % (case.name, counts.tolist()[:16], wc.tolist()[:16])
    real = np.arange(case.k)[None, :] < wc[:, None]
    assert (ids[~real] == PAD).all() and (groups[~real] == PAD).all() and np.array_equal(scores[~real], np.full(int((~real).sum()), -np.inf)), \
        "%s: a padding slot holds something else than (-inf, INT64_MAX, INT64_MAX)" % case.name
    e = eligible(case)
    rows = ids - case.id_base
    inside = (rows >= 0) & (rows < case.N)
    assert inside[real].all(), "%s: a row id outside the index" % case.name
    qq = np.broadcast_to(np.arange(case.Q)[:, None], ids.shape)
    assert e[qq[real], rows[real]].all(), "%s: an ineligible id in a result" % case.name
    assert np.array_equal(groups[real], I["groups"][rows[real]]), "%s: a group column that is not the key of its row" % case.name
    for qi in range(case.Q):
        c = int(wc[qi])
        assert len(set(groups[qi, :c].tolist())) == c, "%s: a group twice in one list" % case.name
        for j in range(c):                                     # the representative is its group's best eligible row
            r = rows[qi, j]
            mates = np.flatnonzero(e[qi] & (I["groups"] == groups[qi, j]))
            best = I["s"][qi, mates].max()
            assert I["s"][qi, r] == best and r == mates[I["s"][qi, mates] == best].min(), \
                "%s: query %d, group %d is not represented by its best eligible row (the lowest among equals)" % (case.name, qi, groups[qi, j])
        if c < 2:
            continue
        d = scores[qi, 1:c] - scores[qi, :c - 1]
        assert (d <= 0).all(), "%s: scores increase along a list" % case.name
        assert (ids[qi, 1:c] > ids[qi, :c - 1])[d == 0].all(), "%s: an exact tie with the higher row first" % case.name
    bad = np.argwhere(ids != wi)
    assert bad.size == 0, "%s: %d ids differ, first at query %d rank %d: got %d, want %d" % (
        case.name, len(bad), bad[0][0], bad[0][1], ids[tuple(bad[0])], wi[tuple(bad[0])])
    assert np.array_equal(groups, wg)
    assert not np.isnan(scores).any()
    worst = float(np.abs(scores[real] - ws[real]).max()) if real.any() else 0.0
    assert worst <= score_bar(case), "%s: score off by %.3e, bar %.3e" % (case.name, worst, score_bar(case))
    return worst
