"""Cases shared by tests/test_gpu_score_biased.py (GPU) and tests/test_biased_cases_host.py (CPU): sse_score_topk_biased, the
exact top-k of score + weight * bias[row] among the tag-eligible rows of the index.  DESIGN K6l.

One list, CASES.  A case takes its index, queries and copy group from a tests/topk_cases.py case and its tags and masks from a
builder of tests/filtered_cases.py; a bias builder adds the per-row bias (float32 [N]) and the per-query weights (float32 [Q],
or None: 1.0 for every query).  inputs(case) builds them from the case's seed, expected(case) is the float64 reference --
O.scores_f64, + float64(w) * float64(bias) formed elementwise (one rounding, as the call defines it), the ineligible columns
removed, O.topk, (-inf, INT64_MAX) padding, counts -- preconditions(case) proves the reference is one the device can be held
to, and check(case, scores, ids, counts) is what every entry point's result must pass.  The counter deltas a call must cause:

  score_biased_bruteforce_queries   +1 per query whose collect buffer (SSE_COLLECT_CAP = 4096 rows) overflowed: `brute`, exact
  score_biased_collected_rows       every row of the answer was re-scored by the select stage: at least the sum of the counts
                                    of the queries the float64 sweep did not take (`collected_min`)

No GPU import here."""
import functools

import numpy as np

from oracle import sse_oracle as O
from tests import filtered_cases as FC
from tests import topk_cases as TC
from tests.topk_cases import BASE, unit  # noqa: F401

COLLECT_CAP = TC.COLLECT_CAP
PAD_ID = FC.PAD_ID
bit = FC.bit


class Case:
    def __init__(self, name, base, k, tags, bias, brute=0, counts=None, same_as_filtered=False, bias_entry="host", why=""):
        self.name, self.base, self.k, self.build, self.bias_build = name, base, k, tags, bias
        self.Q, self.N, self.S, self.id_base, self.upload = base.Q, base.N, base.S, base.id_base, base.upload
        self.brute = brute                        # delta of score_biased_bruteforce_queries per call
        self.counts = counts                      # the counts the case claims (None: all == k)
        self.same_as_filtered = same_as_filtered  # the GPU test also compares with score_topk_filtered of the same handle, byte for byte
        self.bias_entry = bias_entry              # host: index_set_bias | dev: index_set_bias_dev
        self.why = why

    def __repr__(self):
        return self.name


# ---- bias builders: (case, q, t, group, s, tag_eligible, rng) -> (bias float32 [N], weights float32 [Q] or None)

def _randn(rng, n, scale):
    return (scale * rng.standard_normal(n)).astype(np.float32)


def _bb_zero_weight(case, q, t, group, s, e, rng):
    return _randn(rng, case.N, 0.3), np.zeros(case.Q, np.float32)


def _bb_zero_bias(case, q, t, group, s, e, rng):
    return np.zeros(case.N, np.float32), None


def _bb_plain(scale, weights=None):
    def build(case, q, t, group, s, e, rng):
        w = None if weights is None else np.asarray(weights(case), np.float32)
        return _randn(rng, case.N, scale), w
    return build


def _bb_rerank(case, q, t, group, s, e, rng):
    """three rows per query from unbiased ranks 4 k + 5 .. 4 k + 8 lifted by 0.5: above the query's unbiased best"""
    b = _randn(rng, case.N, 0.02)
    order = np.argsort(-s, axis=1, kind="stable")
    for qi in range(case.Q):
        b[order[qi, 4 * case.k + 5:4 * case.k + 8]] = np.float32(0.5)
    return b, None


def _bb_tail(case, q, t, group, s, e, rng):
    b = _randn(rng, case.N, 0.05)
    b[case.N - 1] = np.float32(0.75)          # the one row of the tail tile
    return b, None


def _bb_tie(case, q, t, group, s, e, rng):
    """copies 0 .. 9 carry b0, copies 10 .. 19 b0 - 0.5, copies 20 .. 29 the float next above b0: the planted query returns copies
    20 .. 29 (equal bias: by id), then copies 0 .. 9 (one float ulp of bias below them: no tie)"""
    b = _randn(rng, case.N, 0.01)
    b0 = np.float32(0.125)
    b[group[0:10]] = b0
    b[group[10:20]] = b0 - np.float32(0.5)
    b[group[20:30]] = np.nextafter(b0, np.float32(1.0))
    return b, None


def _bb_overflow(case, q, t, group, s, e, rng):
    """every copy carries -0.25: 4500 bit-equal rows with equal bias are one tie in any arithmetic, 0.75 for the planted query"""
    b = _randn(rng, case.N, 0.003)
    b[group] = np.float32(-0.25)
    return b, None


def _bb_big(case, q, t, group, s, e, rng):
    b = rng.uniform(-1.0, 1.0, case.N)
    b = (b / np.abs(b).max() * 64.0).astype(np.float32)      # bmax = 64, |w| = 1
    return b, None


def _base(name, Q, N, S, k, **kw):
    return TC.Case(name, Q, N, S, min(k, N), seed=kw.pop("seed", 9000 + Q + N + S + k), **kw)


CASES = [
    Case("zero_weight_k10", _base("zw", 5, 3000, 32, 10, seed=9101), 10, FC._b_none, _bb_zero_weight, same_as_filtered=True,
         why="w = 0 for every query: score_topk_filtered's bits"),
    Case("zero_bias_k40", _base("zb", 5, 3000, 32, 40, seed=9101), 40, FC._b_none, _bb_zero_bias, same_as_filtered=True,
         why="an all-zero bias, weight NULL: score_topk_filtered's bits"),
    Case("rerank_is_wrong", _base("rr", 5, 3000, 32, 10), 10, FC._b_none, _bb_rerank,
         why="answer rows ranked beyond 4 k in the unbiased order: no re-rank of an unbiased candidate list passes"),
    Case("per_query_weights", _base("pw", 5, 3000, 32, 10), 10, FC._b_none,
         _bb_plain(0.2, lambda c: (0.0, 0.25, -1.0, 3.0, 1e-3)), why="a weight per query, zero and negative included"),
    Case("with_tags", _base("wt", 5, 3000, 32, 10), 10, FC._b_one_of(8), _bb_plain(0.1), why="one-of-eight tags: eligibility"),
    Case("fewer_than_k", _base("fk", 4, 500, 16, 10), 10, FC._b_fewer, _bb_plain(0.3), counts=(3, 1, 0, 10),
         why="counts 3, 1, 0; padding; theta = -inf"),
    Case("tail_tile_k33", _base("tt", 2, 33, 5, 33, seed=9105), 33, FC._b_tail, _bb_tail, counts=(17, 16),
         why="tail masking with the bias on the last row, S < 8, k = N"),
    Case("tail_tile_k40", _base("tt", 2, 33, 5, 40, seed=9105), 40, FC._b_tail, _bb_tail, counts=(17, 16), why="k > N"),
    Case("q33_nq4", _base("n4", 33, 2000, 64, 40), 40, FC._b_one_of(4, two=True),
         _bb_plain(0.1, lambda c: np.linspace(-1.0, 2.0, c.Q)), why="NQ = 4, partial second query tile, a weight per query"),
    Case("s300_nq2", _base("n2", 40, 700, 300, 40), 40, FC._b_one_of(4, two=True), _bb_plain(0.1), why="NQ = 2"),
    Case("s620_nq1", _base("n1", 40, 700, 620, 40), 40, FC._b_one_of(4, two=True), _bb_plain(0.1), why="NQ = 1 with Q > 32"),
    Case("k1024_half_eligible", _base("k1", 3, 5000, 64, 1024), 1024, FC._b_half, _bb_plain(0.1), why="largest k"),
    Case("tie_by_bias", TC.Case("bt", 9, 2000, 32, 20, kind="tie", seed=11, copies=30, planted=(4,)), 20, FC._b_none, _bb_tie,
         why="bit-equal copies with equal bias tie and order by id; a bias one float ulp apart does not tie"),
    Case("overflow", TC.Case("bo", 8, 6000, 64, 50, kind="dup", seed=14, copies=4500, planted=(3,), ordinary_below=True), 50,
         FC._b_overflow, _bb_overflow, brute=1, why="4500 eligible copies with equal bias > 4096: the float64 sweep applies the bias"),
    Case("big_bias", _base("bb", 5, 3000, 32, 10), 10, FC._b_none, _bb_big, why="|w| bmax = 64: the widened band still certifies"),
    Case("shard_base_dev", _base("sb", 9, 1200, 40, 33, seed=9111, upload="dev", id_base=BASE), 33, FC._b_shard, _bb_plain(0.2),
         bias_entry="dev", why="index_set_dev + index_set_bias_dev: bias indexed by local row, ids global"),
    Case("shard_base_f64", _base("sb", 9, 1200, 40, 33, seed=9111, upload="f64", id_base=BASE), 33, FC._b_shard, _bb_plain(0.2),
         bias_entry="dev", why="float64 index: idx64 branch of wave_exact_dot"),
    Case("folded_splits", _base("fs", 5, 16400, 16, 10), 10, FC._b_sixteen_blocks, _bb_plain(0.1),
         why="513 tiles, 5 queries: 32 index splits share 16 x 256 maxima slots (atomicMax)"),
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(q, t, group, s, tags, any, none, bias, w): arrays or None, read-only.  s: O.scores_f64 with ONE score per group of
    bit-equal rows (filtered_cases._scores)."""
    q0, t0, group = TC.inputs(case.base)
    q, t = q0.copy(), t0.copy()
    rng = np.random.RandomState(case.base.seed + 199)
    if case.build is FC._b_tail:
        FC._b_tail(case, q, t, group, None, np.random.RandomState(0))   # (edits q before the scores are formed)
    s = FC._scores(case, q, t, group)
    d = dict(tags=None, any=None, none=None)
    built = case.build(case, q, t, group, s, rng)
    d.update({k: v for k, v in built.items() if k in d})                # (a builder's exclusion list is not part of this call)
    d.update(q=q, t=t, group=group, s=s)
    bias, w = case.bias_build(case, q, t, group, s, _tag_eligible(case.Q, case.N, d), rng)
    assert bias.dtype == np.float32 and bias.shape == (case.N,) and (w is None or (w.dtype == np.float32 and w.shape == (case.Q,)))
    d.update(bias=bias, w=w)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def _tag_eligible(Q, N, I):
    e = np.ones((Q, N), bool)
    if I["tags"] is not None:
        tg = I["tags"][None, :]
        if I["any"] is not None:
            e &= (I["any"][:, None] == 0) | ((tg & I["any"][:, None]) != 0)
        if I["none"] is not None:
            e &= (tg & I["none"][:, None]) == 0
    return e


def weights(case):
    """the weights as float32 [Q]: 1.0 where the call is handed NULL"""
    w = inputs(case)["w"]
    return np.ones(case.Q, np.float32) if w is None else w


@functools.lru_cache(maxsize=None)
def eligible(case):
    e = _tag_eligible(case.Q, case.N, inputs(case))
    e.setflags(write=False)
    return e


def biased(s, w, bias):
    """sb = score64 + float64(w) * float64(bias): the product of two floats is exact in double, the sum is rounded once"""
    return s + np.asarray(w, np.float32).astype(np.float64)[:, None] * np.asarray(bias, np.float32).astype(np.float64)[None, :]


@functools.lru_cache(maxsize=None)
def biased_scores(case):
    I = inputs(case)
    sb = np.ascontiguousarray(biased(I["s"], weights(case), I["bias"]))
    sb.setflags(write=False)
    return sb


def topk_of(case, sb, k, e=None):
    """(scores [Q,k], ids [Q,k] + id_base, counts [Q]) of a [Q,N] score matrix over the eligible columns, padded"""
    e = eligible(case) if e is None else e
    ws = np.full((case.Q, k), -np.inf)
    wi = np.full((case.Q, k), PAD_ID, np.int64)
    cnt = np.zeros(case.Q, np.int32)
    for qi in range(case.Q):
        cols = np.flatnonzero(e[qi])
        c = min(k, cols.size)
        cnt[qi] = c
        if c:
            ss, ii = O.topk(sb[qi:qi + 1, cols], c)
            ws[qi, :c], wi[qi, :c] = ss[0], cols[ii[0]] + case.id_base
    return ws, wi, cnt


@functools.lru_cache(maxsize=None)
def reference(case, k=None):
    """(scores float64 [Q,k], ids int64 [Q,k], counts int32 [Q]), read-only."""
    out = topk_of(case, biased_scores(case), case.k if k is None else k)
    for a in out:
        a.setflags(write=False)
    return out


def expected(case):
    return reference(case)


def scales(case):
    """(|q| max, |t| max, |w| max * |bias| max, tol): tol bounds how far a device that sums the S products in its own order and
    then adds the exact product w * bias with one rounding can be from the reference: two float64 summation orders
    (filtered_cases.scales) and the final rounding of both, 2^-53 (qn tn + wb) each."""
    I = inputs(case)
    qn = float(np.linalg.norm(I["q"].astype(np.float64), axis=1).max())
    tn = float(np.linalg.norm(np.asarray(I["t"], np.float64), axis=1).max())
    wb = float(np.abs(weights(case).astype(np.float64)).max() * np.abs(I["bias"].astype(np.float64)).max())
    return qn, tn, wb, 2.0 * case.S * 2.0 ** -53 * qn * tn + 2.0 ** -52 * (qn * tn + wb)


def score_bar(case):
    """the filtered bar plus 2^-52 (qn tn + |w| bmax)"""
    qn, tn, wb, _ = scales(case)
    return max(1e-12 * qn * tn, 2.0 * case.S * 2.0 ** -53 * qn * tn) + 2.0 ** -52 * (qn * tn + wb)


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
    q, t, group, bias = I["q"], I["t"], I["group"], I["bias"]
    sb = biased_scores(case)
    tol = scales(case)[3]
    e = eligible(case)
    assert q.shape == (case.Q, case.S) and t.shape == (case.N, case.S) and 1 <= case.k <= 1024
    assert np.isfinite(bias).all() and np.isfinite(weights(case)).all()
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
        # bit-equal rows with equal bias: one biased score in any arithmetic; everything else further apart than 2 tol
        both = in_group[rows[:-1]] & in_group[rows[1:]] & (bias[rows[:-1]] == bias[rows[1:]])
        assert (gap[both] == 0).all()
        if (~both).any():
            assert gap[~both].min() > 2 * tol, "%s query %d: neighbours %.3e apart, 2 tol = %.3e" % (case.name, qi, gap[~both].min(), 2 * tol)
    want_counts = np.minimum(e.sum(1), case.k)
    assert np.array_equal(reference(case)[2], want_counts)
    if case.counts is not None:
        assert tuple(int(c) for c in want_counts) == tuple(case.counts), (case.name, want_counts)
    else:
        assert (want_counts == case.k).all(), (case.name, want_counts)
    if case.same_as_filtered:
        assert np.array_equal(sb.view(np.uint64), I["s"].view(np.uint64)), "the biased scores are not the unbiased bits"
    else:
        assert (reference(case)[1] != topk_of(case, I["s"], case.k)[1]).any(), "the bias changes no answer of the case"
    # overflow: a buffer takes SSE_COLLECT_CAP rows and holds tag-eligible rows only
    if case.brute == 0:
        assert e.sum(1).max() <= COLLECT_CAP, "%s: an overflow the case does not claim is possible" % case.name
    else:
        planted = list(case.base.planted)
        assert len(planted) == case.brute and case.base.ordinary_below and I["w"] is None
        assert len(set(bias[group].tolist())) == 1 and bias[group[0]] < 0
        ordinary = ~in_group
        for p in planted:
            # the eligible copies are bit-equal rows with one bias: their fp32 biased values are one number, their float64 ones
            # another; they are the strict maxima of the planted query's row, so all 4500 are at or above any threshold that
            # keeps k rows: the buffer overflows
            assert e[p, group].all() and group.size > COLLECT_CAP and np.array_equal(wi[p, :case.k] - case.id_base, group[:case.k])
            assert sb[p, group[0]] > sb[p][ordinary & e[p]].max() + 1e-2
        others = np.setdiff1d(np.arange(case.Q), planted)
        # another query never collects a copy: it scores them below zero (and their bias is negative), and its threshold is
        # positive -- a maximum slot of the sweep holds at most 4 rows of this index (188 tiles, 8 splits, 8 waves: 3 tiles per
        # wave, one row of each per slot), so the k-th largest maximum is at least the 4 k-th best eligible biased score, far
        # above twice the bound e_b = e + 2^-23 (|q||t| + e + |w| bmax) < 2e-5
        assert (case.N + 31) // 32 == 188
        for o in others:
            assert sb[o, group[0]] < 0
            best = np.sort(sb[o][e[o]])[::-1]
            assert best[4 * case.k - 1] > 1e-2
            assert int((e[o] & ordinary).sum()) <= COLLECT_CAP
    if case.name == "rerank_is_wrong":
        order = np.argsort(-I["s"], axis=1, kind="stable")
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, np.arange(case.N)[None, :].repeat(case.Q, 0), axis=1)
        got = reference(case)[1] - case.id_base
        for qi in range(case.Q):
            assert (rank[qi, got[qi]] >= 4 * case.k).sum() >= 3, "query %d: no answer row from beyond 4 k" % qi
        rs, ri, rc = rerank_of_unbiased(case, 4 * case.k)
        assert (ri != reference(case)[1]).any(axis=1).all(), "a re-rank of the unbiased top 4 k finds a query's answer"
    if case.name == "tie_by_bias":
        p = case.base.planted[0]
        b = bias[group]
        assert (b[0:10] == b[0]).all() and (b[20:30] == np.nextafter(b[0], np.float32(1))).all() and case.k == 20
        got, gs = reference(case)[1][p] - case.id_base, reference(case)[0][p]
        assert np.array_equal(got, np.concatenate([group[20:30], group[0:10]]))
        assert (gs[:10] == gs[0]).all() and (gs[10:] == gs[10]).all() and 0 < gs[0] - gs[10] < 2e-8   # (one ulp of 0.125f = 2^-26)
    if case.name == "big_bias":
        assert abs(scales(case)[2] - 64.0) < 1e-6
    if case.name.startswith("tail_tile"):
        assert bias[case.N - 1] == np.float32(0.75) and case.N % 32 == 1
    return True


def rerank_of_unbiased(case, m):
    """the defect the call exists to remove: the unbiased top m of the eligible rows, bias added, sorted, cut to k"""
    I = inputs(case)
    e = eligible(case)
    _, ui, uc = topk_of(case, I["s"], m)
    keep = np.zeros((case.Q, case.N), bool)
    for qi in range(case.Q):
        keep[qi, ui[qi, :uc[qi]] - case.id_base] = True
    return topk_of(case, biased_scores(case), case.k, e & keep)


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
        d = scores[qi, 1:c] - scores[qi, :c - 1]
        assert (d <= 0).all(), "%s: scores increase along a list" % case.name
        assert (ids[qi, 1:c] > ids[qi, :c - 1])[d == 0].all(), "%s: an exact tie with the higher row first" % case.name
    return worst
