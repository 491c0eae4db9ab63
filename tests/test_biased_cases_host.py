"""CPU self-test of tests/biased_cases.py, the cases of tests/test_gpu_score_biased.py: every case's preconditions hold, check()
accepts the reference and rejects each defect a biased top-k could produce -- the bias ignored, a re-rank of the unbiased top
4 k, another query's weight, the bias indexed by global id, the bias added in float32, a tie in the wrong order, a padding slot
that holds something -- sse_index.csls_bias agrees with numpy on a stub handle, and the four entry points are declared, bound
and exported."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import biased_cases as BC

ALL = pytest.mark.parametrize("case", BC.CASES, ids=repr)


def _ref(case):
    ws, wi, wc = BC.expected(case)
    return ws.copy(), wi.copy(), wc.copy()


def _rejects(case, scores, ids, counts):
    ws, wi, wc = BC.expected(case)
    assert not (np.array_equal(scores, ws) and np.array_equal(ids, wi) and np.array_equal(counts, wc)), "the defect changed nothing"
    with pytest.raises(AssertionError):
        BC.check(case, scores, ids, counts)


def test_the_list_is_the_one_the_issue_asks_for():
    by = BC.BY_NAME
    shapes = {n: (c.Q, c.N, c.S, c.k) for n, c in by.items()}
    want = dict(zero_weight_k10=(5, 3000, 32, 10), zero_bias_k40=(5, 3000, 32, 40), rerank_is_wrong=(5, 3000, 32, 10),
                tail_tile_k33=(2, 33, 5, 33), tail_tile_k40=(2, 33, 5, 40), k1024_half_eligible=(3, 5000, 64, 1024),
                overflow=(8, 6000, 64, 50), folded_splits=(5, 16400, 16, 10))
    for n, s in want.items():
        assert shapes[n] == s, n
    for n in ("per_query_weights", "with_tags", "fewer_than_k", "q33_nq4", "s300_nq2", "s620_nq1", "tie_by_bias", "big_bias",
              "shard_base_dev", "shard_base_f64"):
        assert n in by
    assert len(by) == len(BC.CASES) and max(c.N for c in BC.CASES) <= 16400
    assert BC.weights(by["per_query_weights"]).tolist() == [np.float32(x) for x in (0, 0.25, -1, 3, 1e-3)]
    assert by["fewer_than_k"].counts == (3, 1, 0, 10)
    assert by["overflow"].brute == 1 and by["overflow"].base.copies == 4500 and sum(c.brute for c in BC.CASES) == 1
    assert by["shard_base_dev"].id_base == by["shard_base_f64"].id_base == BC.BASE
    assert (by["shard_base_dev"].upload, by["shard_base_f64"].upload) == ("dev", "f64")
    assert by["shard_base_dev"].bias_entry == by["shard_base_f64"].bias_entry == "dev"
    assert (by["q33_nq4"].S, by["s300_nq2"].S, by["s620_nq1"].S) == (64, 300, 620) and by["q33_nq4"].Q == 33
    assert [c.name for c in BC.CASES if c.same_as_filtered] == ["zero_weight_k10", "zero_bias_k40"]
    assert not BC.weights(by["zero_weight_k10"]).any() and not BC.inputs(by["zero_bias_k40"])["bias"].any()
    assert BC.inputs(by["zero_bias_k40"])["w"] is None and BC.inputs(by["zero_weight_k10"])["bias"].any()


@ALL
def test_preconditions(case):
    assert BC.preconditions(case)


@ALL
def test_check_accepts_the_reference(case):
    ws, wi, wc = _ref(case)
    assert BC.check(case, ws, wi, wc) == 0.0


@ALL
def test_check_accepts_scores_moved_by_half_the_tolerance(case):
    ws, wi, wc = _ref(case)
    tol = BC.scales(case)[3]
    sign = np.where(ws.view(np.uint64) & np.uint64(1), 1.0, -1.0)
    moved = np.where(np.isfinite(ws), ws + sign * (tol / 2), ws)
    assert BC.check(case, moved, wi, wc) <= tol


@pytest.mark.parametrize("case", [c for c in BC.CASES if not c.same_as_filtered], ids=repr)
def test_check_rejects_the_bias_ignored(case):
    _rejects(case, *BC.topk_of(case, BC.inputs(case)["s"], case.k))


def test_check_rejects_a_rerank_of_the_unbiased_top_4k():
    case = BC.BY_NAME["rerank_is_wrong"]
    _rejects(case, *BC.rerank_of_unbiased(case, 4 * case.k))


@pytest.mark.parametrize("name", ["per_query_weights", "q33_nq4"])
def test_check_rejects_another_querys_weight(name):
    case = BC.BY_NAME[name]
    I = BC.inputs(case)
    _rejects(case, *BC.topk_of(case, BC.biased(I["s"], np.roll(BC.weights(case), 1), I["bias"]), case.k))


@pytest.mark.parametrize("name", ["shard_base_dev", "shard_base_f64"])
def test_check_rejects_the_bias_indexed_by_global_id(name):
    case = BC.BY_NAME[name]
    I = BC.inputs(case)
    wrong = I["bias"][(np.arange(case.N) + case.id_base) % case.N]     # (what a wrapped or offset read would fetch)
    _rejects(case, *BC.topk_of(case, BC.biased(I["s"], BC.weights(case), wrong), case.k))


@pytest.mark.parametrize("name", ["with_tags", "big_bias", "per_query_weights"])
def test_check_rejects_the_bias_added_in_float32(name):
    case = BC.BY_NAME[name]
    I = BC.inputs(case)
    s32 = (I["s"].astype(np.float32) + BC.weights(case)[:, None] * I["bias"][None, :]).astype(np.float64)
    assert s32.dtype == np.float64
    _rejects(case, *BC.topk_of(case, s32, case.k))
    # the product alone rounded to float32, the sum in float64
    prod32 = (BC.weights(case)[:, None] * I["bias"][None, :]).astype(np.float64)
    if name == "per_query_weights":                                    # (|w| = 1 elsewhere: the product is the bias itself)
        _rejects(case, *BC.topk_of(case, I["s"] + prod32, case.k))


def test_check_rejects_a_tie_order_reversed():
    case = BC.BY_NAME["tie_by_bias"]
    p = case.base.planted[0]
    for a, b in ((3, 4), (12, 13)):
        ws, wi, wc = _ref(case)
        assert ws[p, a] == ws[p, b]
        wi[p, [a, b]] = wi[p, [b, a]]
        _rejects(case, ws, wi, wc)
    # the copies one float ulp of bias apart are NOT a tie: id order across them is wrong
    ws, wi, wc = _ref(case)
    order = np.argsort(wi[p], kind="stable")
    _rejects(case, ws[:, :], np.ascontiguousarray(np.where(np.arange(case.Q)[:, None] == p, wi[p][order][None, :], wi)), wc)


@pytest.mark.parametrize("name", ["fewer_than_k", "tail_tile_k40"])
def test_check_rejects_a_padding_slot_that_holds_something(name):
    case = BC.BY_NAME[name]
    e = BC.eligible(case)
    for what in ("id", "score", "zero_row"):
        ws, wi, wc = _ref(case)
        qi = int(np.argmin(wc))
        if what == "id":
            wi[qi, -1] = case.id_base + int(np.flatnonzero(e[qi])[0]) if e[qi].any() else case.id_base
        elif what == "score":
            ws[qi, -1] = 0.0
        else:
            ws[qi, wc[qi]], wi[qi, wc[qi]] = 0.0, case.id_base + case.N    # a zero row behind the last tile
        _rejects(case, ws, wi, wc)


@ALL
def test_check_rejects_a_wrong_count(case):
    for d in (1, -1):
        ws, wi, wc = _ref(case)
        wc[case.Q - 1] += d
        _rejects(case, ws, wi, wc)


class _StubHandle:
    """index_upload / score_topk from the float64 oracle"""

    def __init__(self):
        self.rows, self.calls = None, []

    def index_upload(self, rows, id_base=0):
        self.rows = np.array(rows, np.float32)

    def score_topk(self, q, k):
        self.calls.append((q.shape[0], k))
        return O.topk(O.scores_f64(np.asarray(q, np.float32), self.rows.astype(np.float64)), k)


def csls_inputs(seed=5, N=400, M=300, S=16, hubs=3):
    """(targets [N,S], sources [M,S]) unit rows.  Sources 40 h .. 40 h + 40 crowd around a centre; target h, a "hub", is the
    normalised mean of that crowd -- near every one of its 40 sources -- and target 10 + i is a noisy copy of source i, its
    translation, for the 120 crowded sources: the hub outscores many a translation until the correction takes its share."""
    rng = np.random.RandomState(seed)
    src, tgt = BC.unit(rng, M, S), BC.unit(rng, N, S)

    def norm(x):
        return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)

    for h in range(hubs):
        rows = slice(40 * h, 40 * h + 40)
        src[rows] = norm(src[rows].astype(np.float64) * 0.5 + BC.unit(rng, 1, S).astype(np.float64))
        tgt[h] = norm(src[rows].astype(np.float64).mean(0))
    tgt[10:10 + 40 * hubs] = norm(src[:40 * hubs].astype(np.float64) + 0.6 * BC.unit(rng, 40 * hubs, S).astype(np.float64))
    return tgt, src


def csls_reference(tgt, src, k):
    s = O.scores_f64(tgt, src.astype(np.float64))
    return -0.5 * np.sort(s, axis=1)[:, ::-1][:, :min(k, src.shape[0])].mean(axis=1)


def test_csls_bias_against_numpy_on_a_stub_handle():
    from sse_amd.sse_index import csls_bias
    tgt, src = csls_inputs()
    for k, block in ((10, 4096), (10, 128), (500, 77)):               # k > M: min(k, M)
        h = _StubHandle()
        b = csls_bias(h, tgt, src, k=k, block=block)
        assert b.dtype == np.float32 and b.shape == (tgt.shape[0],)
        assert np.array_equal(h.rows, src), "the handle is left holding the source rows"
        assert sum(c[0] for c in h.calls) == tgt.shape[0] and {c[1] for c in h.calls} == {min(k, src.shape[0])}
        assert max(c[0] for c in h.calls) <= block
        assert np.abs(b.astype(np.float64) - csls_reference(tgt, src, k)).max() <= 1e-6
    # the hubs are what the correction is for: their bias is the most negative, and it changes a query's best row
    b = csls_bias(_StubHandle(), tgt, src)
    assert set(np.argsort(b)[:3].tolist()) == {0, 1, 2}
    s = O.scores_f64(src, tgt.astype(np.float64))
    plain, fixed = np.argmax(s, axis=1), np.argmax(s + b.astype(np.float64)[None, :], axis=1)
    moved = np.flatnonzero(plain != fixed)
    assert moved.size and (plain[moved] < 3).any(), "no query's best target moves off a hub"


def test_the_calls_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    import sse_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sse_hip.h")).read()
    lib = sse_amd.load_library()
    for name in ("sse_index_set_bias", "sse_index_set_bias_dev", "sse_score_topk_biased", "sse_score_topk_biased_dev"):
        assert "int %s(sse_handle *h" % name in header, name
        assert name in sse_amd.SYMBOLS and hasattr(lib, name), name
    for word in ("rounded ONCE", "Cost note", "Out of scope"):
        assert word in header
