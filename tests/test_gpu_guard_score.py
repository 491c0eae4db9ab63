"""Scoring entry points on guarded, skewed caller buffers (tests/guard_bands.py): every pointer argument of
sse_index_set_dev, sse_index_set_tags_dev / _groups_dev / _bias_dev, sse_score_topk_dev, _rank_dev, _above_dev,
_topk_filtered_dev, _topk_grouped_dev, _topk_after_dev, _confusions_dev, _topk_biased_dev, _lse_dev, sse_merge_topk_dev and
sse_merge_topk_strided_dev sits between guards, with no skew and one element off 16-byte alignment, under both fills.

No new reference: the inputs of a shape are tests/lse_cases.py's (unit rows, _t_mixed tags with an empty set, _b_mixed bias
and weights, a device-adopted index with an id_base beyond int32); the float64 scores are its q . t; the expected lists are
O.topk's order (score descending, equal scores by ascending id) with the rows each header rule removes taken out, at the
project's 1e-12; sse_score_above goes through tests/above_cases.py, sse_score_lse through lse_cases.check.  Scores are
float64 and exact by contract, so every output must also be bit-identical to the same call on whole allocations, and to
itself whichever fill surrounded the index when it was adopted."""
import functools

import numpy as np
import pytest

from tests import above_cases as AC
from tests import guard_bands as GB
from tests import lse_cases as LC
from tests import topk_cases as TC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

PAD = np.iinfo(np.int64).max
BAR = 1e-12
INDEXES = [(N, S) for N in (32, 33, 571) for S in (50, 64)]
QS = (1, 5, 33, 129)
# the k of the entries beside sse_score_topk_dev, per Q: every k of the list at two query counts (40 > N at N = 32, 33: k may exceed N there)
OTHER_K = {1: (1, 10), 5: (10, 40), 33: (40, 16), 129: (16, 1)}
F32, F64, I32, I64, U64 = np.float32, np.float64, np.int32, np.int64, np.uint64


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _guard(rows, cols, itemsize):
    """64-row tiles by the width padded to 64, or 128-query blocks by k: the larger of the two, never under 64 KiB"""
    return max(GB.guard_bytes(rows, cols, itemsize, 64, 64), GB.guard_bytes(rows, cols, itemsize, 128, 1))


def _in(a, valid=None, rows=None):
    a = np.ascontiguousarray(a)
    rows = a.shape[0] if rows is None else rows
    return GB.spec(a.dtype, a.size, "in", init=a, valid=valid, guard=_guard(rows, max(a.size // max(rows, 1), 1), a.dtype.itemsize))


def _out(dtype, rows, cols, valid=None, role="out", id_range=None):
    return GB.spec(dtype, rows * cols, role, valid=valid, id_range=id_range, guard=_guard(rows, cols, np.dtype(dtype).itemsize))


class Ref(object):
    pass


@functools.lru_cache(maxsize=None)
def _ref(N, S, Q):
    """Inputs and float64 reference of a shape; read-only."""
    case = LC.Case("guard-n%d-s%d-q%d" % (N, S, Q), Q, N, S, 64, 9000 + N + S, tags=LC._t_mixed, bias=LC._b_mixed, upload="dev",
                   id_base=LC.BASE)
    I = LC.inputs(case)
    r = Ref()
    r.case, r.I, r.N, r.S, r.Q, r.base = case, I, N, S, Q, case.id_base
    r.s = I["q"].astype(np.float64) @ I["t"].astype(np.float64).T
    r.sb = r.s + I["w"].astype(np.float64)[:, None] * I["bias"].astype(np.float64)[None, :]
    r.elig = LC.eligible(case)
    r.groups = ((np.arange(N, dtype=np.int64) * 7919) % max(3, N // 4)) * 4294967311 - 5      # keys beyond 2^32, one negative
    tol = 2.0 * S * 2.0 ** -53 * 1.0001
    for m in (r.s, r.sb):                               # the precondition of topk_cases: no two neighbours within two sums' reach
        gap = -np.diff(-np.sort(-m, axis=1), axis=1)
        assert gap.min() > 2 * tol, "neighbours %.3e apart" % gap.min()
    r.order = np.argsort(-r.s, axis=1, kind="stable")
    r.order_b = np.argsort(-r.sb, axis=1, kind="stable")
    return r


def _lists(order, s, keep, k, base):
    """(scores [Q,k], ids [Q,k], counts [Q]): per query the rows of `order` that `keep` admits, first k; (-inf, PAD) behind"""
    Q = order.shape[0]
    ws, wi, wc = np.full((Q, k), -np.inf), np.full((Q, k), PAD, np.int64), np.zeros(Q, np.int32)
    for q in range(Q):
        rows = order[q][keep[q][order[q]]][:k]
        wc[q] = len(rows)
        ws[q, :len(rows)], wi[q, :len(rows)] = s[q, rows], rows + base
    return ws, wi, wc


def _check_lists(what, o, want, Q, k, counts=True):
    ws, wi, wc = want
    gs, gi = o["scores"].reshape(Q, k), o["ids"].reshape(Q, k)
    assert np.array_equal(gi, wi), "%s: ids differ at %s" % (what, np.argwhere(gi != wi)[:3].tolist())
    live = wi != PAD
    assert np.array_equal(gs[~live], ws[~live]), "%s: the columns behind the count are not (-inf, INT64_MAX)" % what
    assert not live.any() or np.abs(gs[live] - ws[live]).max() <= BAR, what
    if counts:
        assert np.array_equal(o["counts"], wc), what


class Entries(object):
    """One guarded call per entry point on the index the handle holds; every method returns the guarded outputs."""

    def __init__(self, h, be, r, skew):
        self.h, self.be, self.r, self.skew = h, be, r, skew
        self.q = r.I["q"]
        self.idr = (r.base, r.base + r.N, (PAD,))

    def _lists_specs(self, Q, k, **more):
        d = dict(q=_in(self.q), scores=_out(F64, Q, k), ids=_out(I64, Q, k, valid=self.r.base + 1, id_range=self.idr),
                 counts=_out(I32, Q, 1, valid=1))
        d.update(more)
        return d

    def _masks(self):
        return dict(any=_in(self.r.I["any"], valid=1), none=_in(self.r.I["none"], valid=1))

    def topk(self, k):
        r, h, Q = self.r, self.h, self.r.Q
        specs = self._lists_specs(Q, k)
        del specs["counts"]
        want = _lists(r.order, r.s, np.ones((Q, r.N), bool), k, r.base)
        return GB.drive(self.be, specs, lambda b: h.score_topk_dev(b["q"].ptr, Q, k, b["scores"].ptr, b["ids"].ptr), self.skew,
                        lambda o: _check_lists("topk", o, want, Q, k, counts=False))

    def rank(self):
        r, h, Q = self.r, self.h, self.r.Q
        L = 2 * Q
        pq = np.concatenate([np.arange(Q), np.arange(Q)]).astype(I32)
        rows = (np.arange(L) * 37 + 5) % r.N
        want_before = np.array([int(np.flatnonzero(r.order[pq[p]] == rows[p])[0]) for p in range(L)], I64)
        specs = dict(q=_in(self.q), pair_q=_in(pq, valid=0), pair_id=_in(rows.astype(I64) + r.base, valid=r.base + 1),
                     before=_out(I64, L, 1, valid=1), score=_out(F64, L, 1))

        def check(o):
            assert np.array_equal(o["before"], want_before), "rank: counts differ"
            assert np.abs(o["score"] - r.s[pq, rows]).max() <= BAR
        o = GB.drive(self.be, specs, lambda b: h.score_rank_dev(b["q"].ptr, Q, b["pair_q"].ptr, b["pair_id"].ptr, L, None, b["before"].ptr,
                                                                 b["score"].ptr) or h.synchronize(), self.skew, check)
        # the threshold form: the device's own score bits as thresholds, out_score NULL
        specs2 = dict(specs, thr=_in(o["score"]))
        del specs2["score"]
        GB.drive(self.be, specs2, lambda b: h.score_rank_dev(b["q"].ptr, Q, b["pair_q"].ptr, b["pair_id"].ptr, L, b["thr"].ptr,
                                                             b["before"].ptr, None) or h.synchronize(), self.skew,
                 lambda o2: np.testing.assert_array_equal(o2["before"], want_before))

    def above(self):
        r, h, Q = self.r, self.h, self.r.Q
        L = Q
        pq = np.arange(L, dtype=I32)
        cnt = (np.arange(L) % 7) + 2                                        # 2 .. 8 rows per pair: thresholds between neighbours
        srt = -np.sort(-r.s, axis=1)
        thr = 0.5 * (srt[pq, cnt - 1] + srt[pq, cnt])
        want = AC.expected_above(r.s, pq, thr, r.base)
        total = int(want[0][-1])
        assert total == int(cnt.sum()) >= 2
        base = dict(q=_in(self.q), pair_q=_in(pq, valid=0), thr=_in(thr), offsets=_out(I64, L + 1, 1, valid=0))

        def call(cap, lists):
            def f(b):
                h.score_above_dev(b["q"].ptr, Q, b["pair_q"].ptr, b["thr"].ptr, L, cap, b["offsets"].ptr,
                                  b["ids"].ptr if lists else None, b["scores"].ptr if lists else None)
                h.synchronize()
            return f
        fits = dict(base, ids=_out(I64, total, 1, valid=r.base + 1, id_range=(r.base, r.base + r.N, ())), scores=_out(F64, total, 1))
        GB.drive(self.be, fits, call(total, True), self.skew,
                 lambda o: AC.assert_above_equal((o["offsets"], o["ids"], o["scores"]), want, exact_scores=False))
        # cap = total - 1: the offsets are written, the lists stay bitwise as they were (include/sse_hip.h)
        short = dict(base, ids=_out(I64, total - 1, 1, valid=r.base + 1, role="untouched"), scores=_out(F64, total - 1, 1, role="untouched"))
        GB.drive(self.be, short, call(total - 1, True), self.skew, lambda o: np.testing.assert_array_equal(o["offsets"], want[0]))
        GB.drive(self.be, base, call(0, False), self.skew, lambda o: np.testing.assert_array_equal(o["offsets"], want[0]))

    def filtered(self, k):
        r, h, Q = self.r, self.h, self.r.Q
        excl = np.stack([r.order[:, 0] + r.base, np.full(Q, -1), np.full(Q, r.base + r.N + 5)], axis=1).astype(I64)
        keep = r.elig.copy()
        keep[np.arange(Q), r.order[:, 0]] = False
        want = _lists(r.order, r.s, keep, k, r.base)
        specs = self._lists_specs(Q, k, excl=_in(excl, valid=r.base + 2), **self._masks())
        GB.drive(self.be, specs, lambda b: h.score_topk_filtered_dev(b["q"].ptr, Q, k, b["any"].ptr, b["none"].ptr, b["excl"].ptr, 3,
                                                                      b["scores"].ptr, b["ids"].ptr, b["counts"].ptr), self.skew,
                 lambda o: _check_lists("filtered", o, want, Q, k))

    def grouped(self, k):
        r, h, Q = self.r, self.h, self.r.Q
        keep = np.zeros((Q, r.N), bool)                                     # a row stays when it is the first of its group among the eligible
        for q in range(Q):
            seen = set()
            for row in r.order[q]:
                if r.elig[q, row] and r.groups[row] not in seen:
                    seen.add(r.groups[row])
                    keep[q, row] = True
        want = _lists(r.order, r.s, keep, k, r.base)
        wg = np.where(want[1] != PAD, r.groups[np.where(want[1] != PAD, want[1] - r.base, 0)], PAD)
        specs = self._lists_specs(Q, k, groups=_out(I64, Q, k, valid=int(r.groups[1])), **self._masks())

        def check(o):
            _check_lists("grouped", o, want, Q, k)
            assert np.array_equal(o["groups"].reshape(Q, k), wg), "grouped: keys differ"
        GB.drive(self.be, specs, lambda b: h.score_topk_grouped_dev(b["q"].ptr, Q, k, b["any"].ptr, b["none"].ptr, b["scores"].ptr,
                                                                     b["ids"].ptr, b["groups"].ptr, b["counts"].ptr), self.skew, check)

    def after(self, k, first):
        """first: a sse_score_topk_dev result (scores, ids); the cursor is its last column, in the device's own score bits"""
        r, h, Q = self.r, self.h, self.r.Q
        j = first[0].shape[1] - 1
        cur_s, cur_i = np.ascontiguousarray(first[0][:, j]), np.ascontiguousarray(first[1][:, j])
        assert np.array_equal(cur_i - r.base, r.order[:, j])
        keep = r.elig.copy()
        for q in range(Q):
            keep[q, r.order[q, :j + 1]] = False
        want = _lists(r.order, r.s, keep, k, r.base)
        specs = self._lists_specs(Q, k, cur_s=_in(cur_s), cur_i=_in(cur_i, valid=r.base + 1), **self._masks())
        GB.drive(self.be, specs, lambda b: h.score_topk_after_dev(b["q"].ptr, Q, k, b["cur_s"].ptr, b["cur_i"].ptr, b["any"].ptr, b["none"].ptr,
                                                                   b["scores"].ptr, b["ids"].ptr, b["counts"].ptr), self.skew,
                 lambda o: _check_lists("after", o, want, Q, k))

    def confusions(self, k):
        r, h, Q = self.r, self.h, self.r.Q
        pos = np.stack([r.order[:, 1] + r.base, np.full(Q, -1)], axis=1).astype(I64)
        keep = np.ones((Q, r.N), bool)
        keep[np.arange(Q), r.order[:, 1]] = False
        want = _lists(r.order, r.s, keep, k, r.base)
        specs = self._lists_specs(Q, k, pos=_in(pos, valid=r.base + 2), pos_score=_out(F64, Q, 1),
                                  pos_id=_out(I64, Q, 1, valid=r.base + 1, id_range=self.idr))

        def check(o):
            _check_lists("confusions", o, want, Q, k)
            assert np.array_equal(o["pos_id"], pos[:, 0]) and np.abs(o["pos_score"] - r.s[np.arange(Q), r.order[:, 1]]).max() <= BAR
        GB.drive(self.be, specs, lambda b: h.score_confusions_dev(b["q"].ptr, Q, k, b["pos"].ptr, 2, float("inf"), b["scores"].ptr, b["ids"].ptr,
                                                                   b["counts"].ptr, b["pos_score"].ptr, b["pos_id"].ptr), self.skew, check)

    def biased(self, k):
        r, h, Q = self.r, self.h, self.r.Q
        want = _lists(r.order_b, r.sb, r.elig, k, r.base)
        specs = self._lists_specs(Q, k, w=_in(r.I["w"]), **self._masks())
        GB.drive(self.be, specs, lambda b: h.score_topk_biased_dev(b["q"].ptr, Q, k, b["w"].ptr, b["any"].ptr, b["none"].ptr, b["scores"].ptr,
                                                                    b["ids"].ptr, b["counts"].ptr), self.skew,
                 lambda o: _check_lists("biased", o, want, Q, k))

    def lse(self):
        r, h, Q = self.r, self.h, self.r.Q
        specs = dict(q=_in(self.q), w=_in(r.I["w"]), lse=_out(F64, Q, 1), count=_out(I64, Q, 1, valid=1), bound=_out(F64, Q, 1), **self._masks())
        GB.drive(self.be, specs, lambda b: h.score_lse_dev(b["q"].ptr, Q, r.case.scale, b["w"].ptr, b["any"].ptr, b["none"].ptr, b["lse"].ptr,
                                                            b["count"].ptr, b["bound"].ptr), self.skew,
                 lambda o: LC.check(r.case, o["lse"], o["count"], o["bound"]))

    def merge(self, k):
        """three row shards' lists (from the reference, padded with (-inf, INT64_MAX) where a shard has fewer than k rows) ->
        the list of the whole index: the merge moves 64-bit words, so its output is exact."""
        r, h, Q, P = self.r, self.h, self.r.Q, 3
        cuts = [0, r.N // 3, r.N // 3 + 1 + r.N // 2, r.N]
        in_s, in_i = np.empty((P, Q, k)), np.empty((P, Q, k), I64)
        for p in range(P):
            keep = np.zeros((Q, r.N), bool)
            keep[:, cuts[p]:cuts[p + 1]] = True
            in_s[p], in_i[p], _ = _lists(r.order, r.s, keep, k, r.base)
        ws, wi, _ = _lists(r.order, r.s, np.ones((Q, r.N), bool), k, r.base)

        def check(o):
            assert GB.same_bits(o["scores"].reshape(Q, k), ws) and np.array_equal(o["ids"].reshape(Q, k), wi), "merge"
        outs = dict(scores=_out(F64, Q, k), ids=_out(I64, Q, k, valid=r.base + 1, id_range=self.idr))
        GB.drive(self.be, dict(in_s=_in(in_s.reshape(P * Q, k)), in_i=_in(in_i.reshape(P * Q, k), valid=r.base + 1), **outs),
                 lambda b: h.merge_topk_dev(b["in_s"].ptr, b["in_i"].ptr, P, Q, k, b["scores"].ptr, b["ids"].ptr), self.skew, check)
        # one all-gather buffer [P][2][Q][k] of 64-bit words: scores and ids of a shard back to back
        words = np.stack([in_s, in_i.view(F64)], axis=1)
        GB.drive(self.be, dict(words=_in(words.reshape(P * 2 * Q, k)), **outs),
                 lambda b: h.merge_topk_strided_dev(b["words"].ptr, b["words"].ptr + Q * k * 8, 2 * Q * k, P, Q, k, b["scores"].ptr, b["ids"].ptr),
                 self.skew, check)


def _adopt(h, be, r, skew, fill):
    """index, tags, group keys and bias through their _dev forms from guarded arrays under one fill"""
    N, S, I = r.N, r.S, r.I
    one = dict(fills=(fill,))
    GB.run_guarded(be, dict(rows=_in(I["t"])), lambda b: h.index_set_dev(b["rows"].ptr, N, S, id_base=r.base), skew, **one)
    GB.run_guarded(be, dict(tags=_in(I["tags"], valid=1, rows=N)), lambda b: h.index_set_tags_dev(b["tags"].ptr, N), skew, **one)
    GB.run_guarded(be, dict(groups=_in(r.groups, valid=int(r.groups[1]), rows=N)), lambda b: h.index_set_groups_dev(b["groups"].ptr, N), skew, **one)
    GB.run_guarded(be, dict(bias=_in(I["bias"], rows=N)), lambda b: h.index_set_bias_dev(b["bias"].ptr, N), skew, **one)


def _all_entries(h, be, r, skew):
    """Every entry at the shape's two k (sse_score_topk_dev at the whole k list); {label: outputs} for the cross-fill identity"""
    e, N = Entries(h, be, r, skew), r.N
    got = {}
    for k in (1, 10, 16, 40, N):
        if k <= N:
            got["topk%d" % k] = e.topk(k)
    e.rank()
    e.above()
    e.lse()
    for kk in OTHER_K[r.Q]:
        kf = min(kk, 16)
        first = got["topk%d" % kf]
        e.filtered(kk)
        e.grouped(kk)
        e.after(kk, (first["scores"].reshape(r.Q, kf), first["ids"].reshape(r.Q, kf)))
        e.confusions(kk)
        e.biased(kk)
        e.merge(min(kk, N))
    return got


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("N,S", INDEXES)
def test_every_scoring_entry_on_guarded_buffers(N, S, skew):
    be = GB.TorchBackend()
    h = _scorer()
    calls = GB.run_guarded.calls
    for Q in QS:
        r = _ref(N, S, Q)
        by_fill = []
        for fill in GB.FILLS:                          # what surrounded the index when it was adopted must not matter either
            _adopt(h, be, r, skew, fill)
            by_fill.append(_all_entries(h, be, r, skew))
        for label in by_fill[0]:
            for name in by_fill[0][label]:
                assert GB.same_bits(by_fill[0][label][name], by_fill[1][label][name]), (label, name, "index adopted under another fill")
    print("GUARDCALLS score %d" % (GB.run_guarded.calls - calls))
    h.close()


# The routes a small shape cannot reach: the small-index scorer, bf16 candidates, the two-pass ranking (its row threshold lowered
# as tests/test_gpu_score.py lowers it).  sse_score_topk_dev alone, held by topk_cases.check.
ROUTES = {
    "small-index": (TC.Case("guard_small_index", 1030, 17, 249, 10, upload="dev", seed=7247), {}, None),
    # S % 4 == 0: with a skewed query pointer it is the POINTER clause of the scorer's `vec` test that picks the scalar loads
    # (score_topk.hip, score_small_index_kernel and its split-bf16 twin), not the shape
    "small-index-s64-fp32": (TC.Case("guard_small_index_s64", 1100, 571, 64, 10, upload="dev", seed=7311), dict(score_small_x3=0), None),
    "small-index-s64-x3": (TC.Case("guard_small_index_s64", 1100, 571, 64, 10, upload="dev", seed=7311), dict(score_small_x3=1), None),
    "bf16": (TC.Case("guard_bf16", 300, 9000, 64, 10, upload="dev", seed=9300), dict(score_bf16=1), None),
    "two-pass": (TC.Case("guard_two_pass", 1100, 9000, 64, 16, upload="dev", seed=10100),
                 dict(score_bf16=1, score_two_pass_rows=524288, score_two_pass_min_rows=0), "score_two_pass_calls"),
}


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_topk_routes_of_larger_shapes_on_guarded_buffers(route, skew):
    case, options, counter = ROUTES[route]
    TC.preconditions(case)
    q, t, _ = TC.inputs(case)
    be = GB.TorchBackend()
    h = _scorer()
    for name, value in options.items():
        h.set_option(name, value)
    Q, k, N, S = case.Q, case.k, case.N, case.S
    calls = GB.run_guarded.calls
    GB.run_guarded(be, dict(rows=_in(t)), lambda b: h.index_set_dev(b["rows"].ptr, N, S, id_base=case.id_base), skew)
    before = h.get_counter(counter) if counter else 0
    specs = dict(q=_in(q), scores=_out(F64, Q, k), ids=_out(I64, Q, k, valid=1, id_range=(0, N, ())))
    GB.drive(be, specs, lambda b: h.score_topk_dev(b["q"].ptr, Q, k, b["scores"].ptr, b["ids"].ptr), skew,
             lambda o: TC.check(case, o["scores"].reshape(Q, k), o["ids"].reshape(Q, k)))
    if counter:
        assert h.get_counter(counter) - before == 3, "the route under test did not run on every call"
    print("GUARDCALLS score %d" % (GB.run_guarded.calls - calls))
    h.close()
