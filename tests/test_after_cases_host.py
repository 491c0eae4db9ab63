"""CPU self-test of tests/after_cases.py, the cases of tests/test_gpu_score_after.py: every case's preconditions hold, check()
accepts the reference and rejects each defect a paged top-k could produce -- a row before the cursor, the cursor row itself, a
skipped row, the higher id first in a tie, a wrong count, dirty padding -- and the layers above the library (sse_index.ranked_pages
/ ranked_rows, the ShardedIndex merge, the cursor arguments of the serving routes) do what they say on a handle built on the
float64 oracle."""
import json

import numpy as np
import pytest

from tests import after_cases as AC

ALL = pytest.mark.parametrize("case", AC.CASES, ids=repr)
STEPS = [(c, st) for c in AC.CASES for st in AC.steps(c)]
ALL_STEPS = pytest.mark.parametrize("case,step", STEPS, ids=lambda x: repr(x))


def _ref(case, step):
    ws, wi, wc = AC.expected(case, step)
    return ws.copy(), wi.copy(), wc.copy()


def _rejects(case, step, scores, ids, counts):
    ws, wi, wc = AC.expected(case, step)
    assert not (np.array_equal(scores, ws) and np.array_equal(ids, wi) and np.array_equal(counts, wc)), "the defect changed nothing"
    with pytest.raises(AssertionError):
        AC.check(case, step, scores, ids, counts)


def test_the_list_is_the_one_the_issue_asks_for():
    by = AC.BY_NAME
    shapes = {(c.Q, c.N, c.S) for c in AC.CASES}
    for shape in [(5, 3000, 32), (5, 700, 32), (3, 2000, 32), (33, 700, 64), (40, 700, 300), (40, 700, 620), (3, 5000, 64), (8, 6000, 64)]:
        assert shape in shapes, shape
    assert len({c.name for c in AC.CASES}) == len(AC.CASES)
    assert [st.k for st in AC.steps(by["first_page_k10"])] == [10, 10] and [st.k for st in AC.steps(by["first_page_k40"])] == [40, 40]
    assert AC.steps(by["first_page_k10"])[1].cursors is None
    ch = AC.steps(by["chain_k33"])
    assert len(ch) == 23 and all(st.k == 33 for st in ch) and by["chain_k33"].N % 32 == 28
    assert [int(AC.expected(by["chain_k33"], st)[2][0]) for st in ch] == [33] * 21 + [7, 0]
    assert by["ties"].base.copies == 30 and [st.label for st in AC.steps(by["ties"])][1:] == ["tenth_copy", "between_two_copies", "int64_max", "int64_min"]
    assert AC.inputs(by["band"])["band"].size == 200
    assert (by["between_dev_base"].upload, by["between_f64_base"].upload) == ("dev", "f64") and by["between_dev_base"].id_base == AC.BASE
    few = by["few_left"]
    assert [AC.expected(few, st)[2].tolist() for st in AC.steps(few)[:5]] == [[3] * 4, [1] * 4, [0] * 4, [0] * 4, [0] * 4]
    assert AC.expected(few, AC.steps(few)[5])[2].tolist() == [10, 10, 0, 10]
    assert by["tags_sorted"].variants == (("skip_on", 1), ("skip_off", 0))
    assert [st.k for st in AC.steps(by["k1024"])] == [1024, 1024]
    ov = by["overflow"]
    assert ov.base.copies == 4500 and [st.brute for st in AC.steps(ov)] == [1, 1] and sum(st.brute for c in AC.CASES for st in AC.steps(c)) == 2


@ALL
def test_preconditions(case):
    assert AC.preconditions(case)


def test_the_constructions_reach_what_they_are_meant_to():
    # ties: the copies' score with four ids -- 20 copies left, 20 again (the id between is no copy), none, all 30
    c = AC.BY_NAME["ties"]
    group, p = AC.inputs(c)["group"], c.base.planted[0]
    st = AC.steps(c)
    assert np.array_equal(AC.expected(c, st[1])[1][p, :20], group[10:]) and np.array_equal(AC.expected(c, st[2])[1][p, :20], group[10:])
    assert not np.isin(AC.expected(c, st[3])[1][p], group).any() and np.array_equal(AC.expected(c, st[4])[1][p, :30], group)
    # overflow: copies 2001 .. 2050
    c = AC.BY_NAME["overflow"]
    group, p = AC.inputs(c)["group"], c.base.planted[0]
    assert np.array_equal(AC.expected(c, AC.steps(c)[1])[1][p], group[2000:2050])
    # best rows ineligible: a cursor inside the ineligible top 100 changes nothing
    c = AC.BY_NAME["tags_best_rows_ineligible"]
    st = AC.steps(c)
    assert np.array_equal(AC.expected(c, st[0])[1], AC.expected(c, st[2])[1])
    # k1024: the second page is ranks 1024 .. 2047
    c = AC.BY_NAME["k1024"]
    assert np.array_equal(AC.expected(c, AC.steps(c)[1])[1], AC.order(c)[:, 1024:2048])
    # a chain built from the oracle's own scores is the whole ranking
    c = AC.BY_NAME["chain_k33"]
    cat = np.concatenate([AC.expected(c, st)[1][:, :AC.expected(c, st)[2][0]] for st in AC.steps(c)], axis=1)
    assert np.array_equal(cat, AC.order(c))
    # cursor_arrays: midpoints are strictly between their neighbours, device scores come from `known`
    c = AC.BY_NAME["band"]
    cs, ci = AC.cursor_arrays(c, AC.steps(c)[0], None)
    s, o = AC.inputs(c)["s"], AC.order(c)
    for qi, cur in enumerate(AC.cursors_of(c, AC.steps(c)[0])):
        assert s[qi, o[qi, cur[1] + 1]] < cs[qi] < s[qi, o[qi, cur[1]]]
    c = AC.BY_NAME["ties"]
    with pytest.raises(AssertionError):
        AC.cursor_arrays(c, AC.steps(c)[1], [dict() for _ in range(c.Q)])
    cs, ci = AC.cursor_arrays(c, AC.steps(c)[3], AC.oracle_known(c, 1))
    assert ci[c.base.planted[0]] == AC.I64_MAX and cs[c.base.planted[0]] == s_of(c)[c.base.planted[0], AC.inputs(c)["group"][0]]


def s_of(case):
    return AC.inputs(case)["s"]


@ALL_STEPS
def test_check_accepts_the_reference(case, step):
    assert AC.check(case, step, *_ref(case, step)) == 0.0


def _first_with(pred):
    for c, st in STEPS:
        if pred(c, st):
            return c, st
    raise AssertionError("no such step")


def _dev_steps():
    """steps with a finite cursor and a full answer for query 0"""
    out = []
    for c, st in STEPS:
        cur = AC.cursors_of(c, st)
        if cur is not None and cur[0][0] in ("mid", "dev") and AC.expected(c, st)[2][0] == st.k and st.k >= 4:
            out.append((c, st))
    return out


@pytest.mark.parametrize("case,step", _dev_steps()[::3], ids=lambda x: repr(x))
def test_check_rejects_rows_on_the_wrong_side_and_skipped_rows(case, step):
    o = AC.order(case)[0]
    am, e = AC.after_mask(case, step)[0], AC.eligible(case)[0]
    before = o[~am[o] & e[o]]
    assert before.size
    # a row before the cursor: the nearest one (for a "dev" cursor with its own id: the cursor row itself) leads the list
    ws, wi, wc = _ref(case, step)
    ws[0, 1:], wi[0, 1:] = ws[0, :-1].copy(), wi[0, :-1].copy()
    ws[0, 0], wi[0, 0] = s_of(case)[0, before[-1]], before[-1] + case.id_base
    _rejects(case, step, ws, wi, wc)
    cur = AC.cursors_of(case, step)[0]
    if cur[0] == "dev" and cur[2] is None:
        assert before[-1] == o[cur[1]]                        # the cursor row itself
    # a skipped row: the list starts one row late
    w1 = AC.expected(case, AC.Step("k+1", step.k + 1, step.cursors))
    if w1[2][0] == step.k + 1:
        ws, wi, wc = _ref(case, step)
        ws[0], wi[0] = w1[0][0, 1:], w1[1][0, 1:]
        _rejects(case, step, ws, wi, wc)
        ws, wi, wc = _ref(case, step)                         # ... or a row is missing in the middle
        j = step.k // 2
        ws[0, j:], wi[0, j:] = w1[0][0, j + 1:], w1[1][0, j + 1:]
        _rejects(case, step, ws, wi, wc)


def test_check_rejects_the_cursor_row_itself():
    case = AC.BY_NAME["chain_k33"]
    step = AC.steps(case)[3]
    prev = AC.expected(case, AC.steps(case)[2])
    ws, wi, wc = _ref(case, step)
    ws[:, 1:], wi[:, 1:] = ws[:, :-1].copy(), wi[:, :-1].copy()
    ws[:, 0], wi[:, 0] = prev[0][:, -1], prev[1][:, -1]
    _rejects(case, step, ws, wi, wc)


def test_check_rejects_two_tied_ids_swapped():
    for name, j in (("ties", 1), ("overflow", 1)):
        case = AC.BY_NAME[name]
        step = AC.steps(case)[j]
        p = case.base.planted[0]
        ws, wi, wc = _ref(case, step)
        assert ws[p, 3] == ws[p, 4]
        wi[p, [3, 4]] = wi[p, [4, 3]]
        _rejects(case, step, ws, wi, wc)


@ALL_STEPS
def test_check_rejects_a_wrong_count(case, step):
    for d in (1, -1):
        ws, wi, wc = _ref(case, step)
        wc[case.Q - 1] += d
        _rejects(case, step, ws, wi, wc)


def test_check_rejects_a_padding_slot_that_holds_something():
    case = AC.BY_NAME["few_left"]
    for step in AC.steps(case):
        for what in ("id", "score", "zero_row"):
            ws, wi, wc = _ref(case, step)
            qi = int(np.argmin(wc))
            if what == "id":
                wi[qi, -1] = case.id_base
            elif what == "score":
                ws[qi, -1] = 0.0
            else:
                ws[qi, wc[qi]], wi[qi, wc[qi]] = 0.0, case.id_base + case.N
            _rejects(case, step, ws, wi, wc)


def test_check_rejects_a_score_off_by_1e_9_and_wrong_types():
    case, step = _first_with(lambda c, st: c.name == "tags_one_of_eight" and st.label == "page1")
    ws, wi, wc = _ref(case, step)
    ws[0, 0] += 1e-9
    _rejects(case, step, ws, wi, wc)
    ws, wi, wc = _ref(case, step)
    with pytest.raises(AssertionError):
        AC.check(case, step, ws.astype(np.float32), wi, wc)
    with pytest.raises(AssertionError):
        AC.check(case, step, ws, wi, wc.astype(np.int64))
    with pytest.raises(AssertionError):
        AC.check(case, step, ws[:, :5], wi[:, :5], wc)


# ---- the layers above the library on an oracle handle

def test_ranked_pages_and_ranked_rows_on_the_oracle():
    from sse_amd.sse_index import ranked_pages, ranked_rows
    case = AC.BY_NAME["ties"]
    I = AC.inputs(case)
    h = AC.OracleHandle(I["t"], id_base=17)
    fs, fi = h.score_topk(I["q"], case.N)
    pages = list(ranked_pages(h, I["q"], 300))
    assert [p[2].tolist() for p in pages] == [[300] * case.Q] * 6 + [[200] * case.Q] and h.calls == 7
    assert np.array_equal(np.concatenate([p[0][:, :p[2][0]] for p in pages], axis=1), fs)
    assert np.array_equal(np.concatenate([p[1][:, :p[2][0]] for p in pages], axis=1), fi)      # through the 30 tied rows too
    pages = list(ranked_pages(h, I["q"], 1000))               # N a multiple of the page: the empty page is not yielded
    assert [int(p[2][0]) for p in pages] == [1000, 1000]
    for k_total, page in ((1, 1024), (450, 200), (2000, 1024), (5000, 256), (0, 10)):
        rs, ri = ranked_rows(h, I["q"], k_total, page=page)
        n = min(k_total, case.N)
        assert np.array_equal(np.stack(rs), fs[:, :n]) and np.array_equal(np.stack(ri), fi[:, :n])
    assert list(ranked_pages(h, np.zeros((0, case.S), np.float32), 10)) == []
    # tagged: lists of different lengths, a query that runs out early keeps count 0
    tcase = AC.BY_NAME["tags_one_of_eight"]
    T = AC.inputs(tcase)
    h = AC.OracleHandle(T["t"], tags=T["tags"])
    fs, fi = h.score_topk(T["q"], tcase.N)
    e = AC.eligible(tcase)
    got = [[] for _ in range(tcase.Q)]
    for sc, ids, cnt in ranked_pages(h, T["q"], 64, any_of=T["any"]):
        for qi in range(tcase.Q):
            got[qi].extend(ids[qi, :cnt[qi]].tolist())
            assert (ids[qi, cnt[qi]:] == AC.PAD_ID).all()
    lengths = set()
    for qi in range(tcase.Q):
        assert got[qi] == fi[qi, e[qi, fi[qi]]].tolist()
        lengths.add(len(got[qi]))
    assert len(lengths) > 1


class _ShardHandle(AC.OracleHandle):
    """the two device entry points ShardedIndex.score_topk_after calls, on CPU tensors' memory"""

    @staticmethod
    def _view(ptr, dtype, n):
        import ctypes
        return np.frombuffer((ctypes.c_char * (n * 8)).from_address(ptr), dtype=dtype, count=n)

    def score_topk_after_dev(self, q_ptr, Q, k, cs_ptr, ci_ptr, any_ptr, none_ptr, s_ptr, i_ptr, c_ptr, stream=0):
        import ctypes
        S = self.t.shape[1]
        q = np.frombuffer((ctypes.c_char * (Q * S * 4)).from_address(q_ptr), dtype=np.float32, count=Q * S).reshape(Q, S)
        after = (self._view(cs_ptr, np.float64, Q), self._view(ci_ptr, np.int64, Q)) if cs_ptr else None
        any_ = self._view(any_ptr, np.uint64, Q) if any_ptr else None
        sc, ids, cnt = self.score_topk_after(q, k, after=after, any_of=any_)
        self._view(s_ptr, np.float64, Q * k)[:] = sc.reshape(-1)
        self._view(i_ptr, np.int64, Q * k)[:] = ids.reshape(-1)
        np.frombuffer((ctypes.c_char * (Q * 4)).from_address(c_ptr), dtype=np.int32, count=Q)[:] = cnt

    def merge_topk_strided_dev(self, in_s, in_i, stride, P, Q, k, out_s, out_i, stream=0):
        s = np.stack([self._view(in_s + 8 * stride * p, np.float64, Q * k).reshape(Q, k) for p in range(P)], axis=1).reshape(Q, P * k)
        i = np.stack([self._view(in_i + 8 * stride * p, np.int64, Q * k).reshape(Q, k) for p in range(P)], axis=1).reshape(Q, P * k)
        o = np.lexsort((i, -s), axis=1)[:, :k]
        self._view(out_s, np.float64, Q * k)[:] = np.take_along_axis(s, o, 1).reshape(-1)
        self._view(out_i, np.int64, Q * k)[:] = np.take_along_axis(i, o, 1).reshape(-1)


def test_sharded_merge_on_oracle_handles(monkeypatch):
    """three shards in one process: the collectives are replaced by ones that hand every rank the lists all ranks produced
    (each rank's local list does not depend on the others', so a first round records them and a second round merges)"""
    import torch
    import torch.distributed as dist
    from sse_amd import collectives
    from sse_amd.sharded import ShardedIndex, shard_bounds
    case = AC.BY_NAME["ties"]
    I = AC.inputs(case)
    world, N, k = 3, case.N, 40
    bounds = shard_bounds(N, world)
    tags = (AC.bit(0) << (np.arange(N) % 3).astype(np.uint64)).astype(np.uint64)
    any_ = np.where(np.arange(case.Q) % 2 == 0, AC.bit(0) | AC.bit(1), np.uint64(0)).astype(np.uint64)
    whole = AC.OracleHandle(I["t"], tags=tags)
    first = whole.score_topk_after(I["q"], k, any_of=any_)
    cs, ci = first[0][:, 9].copy(), first[1][:, 9].copy()       # the tenth entry: inside the 30 copies for the planted query
    cs[1], cs[2] = np.inf, np.nan
    want = whole.score_topk_after(I["q"], k, after=(cs, ci), any_of=any_)
    assert want[2][2] == 0 and (want[2][[0, 1, 3, 4]] == k).all()
    state = {"loc": {}, "cnt": {}, "rank": None, "round": 0}
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: world)

    def all_gather_into(g, loc, group=None, async_op=False):
        state["loc"][state["rank"]] = loc.clone()
        if state["round"] == 1:
            g.copy_(torch.cat([state["loc"][r] for r in range(world)], 0))

    def all_reduce_(total, group=None):
        state["cnt"][state["rank"]] = total.clone()
        if state["round"] == 1:
            total.copy_(sum(state["cnt"][r] for r in range(world)))

    monkeypatch.setattr(collectives, "all_gather_into", all_gather_into)
    monkeypatch.setattr(collectives, "all_reduce_", all_reduce_)
    q = torch.from_numpy(np.array(I["q"]))
    for rnd in (0, 1):
        state["round"] = rnd
        for r, (a, b) in enumerate(bounds):
            state["rank"] = r
            sh = ShardedIndex(_ShardHandle(I["t"][a:b], id_base=a, tags=tags[a:b]), r, world, N)
            sc, ids, cnt = sh.score_topk_after(q, k, after=(torch.from_numpy(cs.copy()), torch.from_numpy(ci.copy())),
                                               any_of=torch.from_numpy(any_.view(np.int64).copy()))
            if rnd == 1:
                assert np.array_equal(ids.numpy(), want[1]) and np.array_equal(sc.numpy(), want[0]), r
                assert np.array_equal(cnt.numpy(), want[2]) and cnt.dtype == torch.int32
    with pytest.raises(ValueError):
        sh.score_topk_after(q, 1025)
    with pytest.raises(ValueError):
        sh.score_topk_after(q, k, after=(torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int64)))


def test_cursor_arguments_of_handle_request():
    from sse_amd import sse_serving
    assert sse_serving.parse_cursor({"query": "x"}) is None
    assert sse_serving.parse_cursor({"after_score": "0.1", "after_id": "-5"}) == (0.1, -5)
    for v in (0.1, 1 / 3, -2.5e-300, 123456.789e10):
        assert sse_serving.parse_cursor({"after_score": repr(v), "after_id": "7"})[0] == v
        assert json.loads(json.dumps({"s": v}))["s"] == v
    assert sse_serving.parse_cursor({"after_score": "inf", "after_id": "0"})[0] == np.inf
    for bad in ({"after_score": "1"}, {"after_id": "1"}, {"after_score": "x", "after_id": "1"}, {"after_score": "1", "after_id": "1.5"}):
        with pytest.raises(ValueError):
            sse_serving.parse_cursor(bad)
    calls = []

    def rank_fn(tokens, nbest, normalize, after=None):
        calls.append((nbest, normalize, after))
        if after is None:
            return [(1.0 - 0.1 * j, "id%d" % j, "name %d" % j) for j in range(nbest)]
        n = 0 if after[1] == 99 else nbest
        return [(after[0] - 0.1 * (j + 1), "id%d" % (after[1] + j + 1), "n", after[1] + j + 1) for j in range(n)]

    tok = lambda text: [1]                                    # noqa: E731
    st, plain = sse_serving.handle_request("/api/search", {"query": "x", "nbest": "3"}, rank_fn, tok)
    assert st == 200 and set(plain) == {"SearchQuery", "SearchRankingResults"} and calls[-1] == (3, False, None)
    st, d = sse_serving.handle_request("/api/search", {"query": "x", "nbest": "3", "after_score": "0.7", "after_id": "4"}, rank_fn, tok)
    assert st == 200 and calls[-1] == (3, False, (0.7, 4))
    assert [r["ListingId"] for r in d["SearchRankingResults"]] == ["id5", "id6", "id7"]
    assert (d["next_after_score"], d["next_after_id"]) == (0.7 - 0.1 * 3, 7)
    st, d = sse_serving.handle_request("/api/classify", {"keywords": "x", "after_score": "0.7", "after_id": "99"}, rank_fn, tok)
    assert st == 200 and d["ClassificationResults"] == [] and (d["next_after_score"], d["next_after_id"]) == (0.7, 99)
    assert calls[-1] == (8, True, (0.7, 99))
    for bad in ({"after_score": "0.7"}, {"after_id": "4"}, {"after_score": "zero", "after_id": "4"}):
        st, body = sse_serving.handle_request("/api/qna", dict(question="x", **bad), rank_fn, tok)
        assert st == 400 and "cursor" in body
