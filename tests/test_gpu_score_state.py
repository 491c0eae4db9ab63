"""The scoring state a long-lived handle keeps from call to call -- the resident index in its images (idxp, idx64, idx_rm,
idx_x3, idxp16), idx_norm_max, idx_base, tags / tile sums / group keys, the grow-only scratch the entry points share, the
zero-once device counters, the pinned mirror block and score_seq -- against a FRESH handle (DESIGN K6, "per-index state").

One test per transition of tests/score_state_script.py; each drives one long-lived handle through a script.  For every call:
  (a) a fresh handle that holds only the current index, tags, keys and options makes this one call: every output array has
      the same bits (padding slots, counts, offsets included) and every score_* counter of sse_get_counter moves by the same
      amount -- a stale image that the scorer's certificates heal shows up here and nowhere else;
  (b) the float64 oracle (StateOracle of the script, proven on the CPU by tests/test_score_state_host.py): ids, counts,
      offsets, padding exact, scores within topk_cases.score_bar's formula;
  (c) the host form and the device-pointer forms (outputs pre-filled with NaN / -7) return the same bits.
No counter is exempted from (a).  One SCORESTATE line per call (profiles/score_state.txt)."""
import numpy as np
import pytest

from tests import score_state_script as SS
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

PARAMS = model_params("dual-encoder", 50, 8, 16, 16, 8, 4)

# every counter named score_* in the table of sse_get_counter (csrc/sse_api.hip, COUNTERS)
NAMES = ("score_two_pass_calls", "score_rank_band_rows", "score_rank_bruteforce_pairs", "score_above_band_rows",
         "score_above_bruteforce_pairs", "score_above_long_segments", "score_filtered_collected_rows",
         "score_filtered_bruteforce_queries", "score_filtered_tiles_skipped", "score_grouped_collected_rows",
         "score_grouped_bruteforce_queries", "score_after_collected_rows", "score_after_bruteforce_queries",
         "score_bf16_second_chance_queries", "score_collect_queries", "score_bruteforce_queries")
EXEMPT = ()


class GpuDriver:
    """sse_amd's Handle behind the driver interface of the script"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.m, _ = make_pair(PARAMS)
        self.h = self.m.handle
        self.rows = None
        self.stream = None

    def close(self):
        self.h.close()

    # -- state
    def _up(self, x, dtype):
        return None if x is None else self.torch.from_numpy(np.array(x, dtype=dtype)).to(self.dev)

    def _words(self, x):
        return None if x is None else self.torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).to(self.dev)

    def _guard(self, fn, *a, **kw):
        import sse_amd
        try:
            return fn(*a, **kw)
        except sse_amd.SSEError as e:
            raise SS.Refused(str(e))

    def set_index(self, rows, how, id_base):
        if how in ("f32", "f64"):
            assert rows.dtype == (np.float64 if how == "f64" else np.float32)
            self._guard(self.h.index_upload, rows, id_base=id_base)
            return
        N, S = rows.shape
        flat = self.torch.zeros(N * S + 4, dtype=self.torch.float32, device=self.dev)
        off = 1 if how == "dev_unaligned" else 0            # 4 bytes past the allocation's (at least 16-byte) boundary
        d = flat[off:off + N * S]
        d.copy_(self.torch.from_numpy(np.array(rows, dtype=np.float32).reshape(-1)))
        assert d.data_ptr() % 16 == (4 if off else 0)
        self.torch.cuda.synchronize()
        self._guard(self.h.index_set_dev, d.data_ptr(), N, S, id_base=id_base)
        self.torch.cuda.synchronize()
        self.rows = flat

    def set_tags(self, words, dev=False):
        if dev and words is not None:
            d = self._words(words)
            self._guard(self.h.index_set_tags_dev, d.data_ptr(), len(words))
            self.torch.cuda.synchronize()
        else:
            self._guard(self.h.index_set_tags, words)

    def set_groups(self, keys, dev=False):
        if dev and keys is not None:
            d = self._up(keys, np.int64)
            self._guard(self.h.index_set_groups_dev, d.data_ptr(), len(keys))
            self.torch.cuda.synchronize()
        else:
            self._guard(self.h.index_set_groups, keys)

    def set_option(self, name, value):
        self._guard(self.h.set_option, name, value)

    def counters(self, names):
        return tuple(self.h.get_counter(n) for n in names)

    # -- host forms
    def _host(self, entry, a):
        h = self.h
        if entry == "topk":
            return h.score_topk(a["q"], a["k"])
        if entry == "rank":
            return h.score_rank(a["q"], a["pair_q"], a["pair_id"], a.get("pair_score"))
        if entry == "count_above":
            return (h.count_above(a["q"], a["thr"], a["pair_q"]),)
        if entry == "above":
            off, ids, sc = h.score_above(a["q"], a["thr"], a["pair_q"], cap=a["cap"])
            return (off, np.zeros(0, np.int64), np.zeros(0, np.float64)) if ids is None else (off, ids, sc)
        if entry == "filtered":
            return h.score_topk_filtered(a["q"], a["k"], a.get("any_of"), a.get("none_of"), a.get("exclude"))
        if entry == "grouped":
            return h.score_topk_grouped(a["q"], a["k"], a.get("any_of"), a.get("none_of"))
        if entry == "after":
            return h.score_topk_after(a["q"], a["k"], a.get("after"), a.get("any_of"), a.get("none_of"))
        if entry == "encode_topk":
            return h.encode_score_topk(0, a["ids"], True, a["k"], want_encodings=True)
        raise ValueError(entry)

    # -- device forms: inputs uploaded, outputs pre-filled, the call queued on stream s; nothing is read here
    def _enqueue(self, entry, a, s):
        T, h = self.torch, self.h
        f64, i64, i32 = T.float64, T.int64, T.int32

        def full(shape, fill, dtype):
            return T.full(shape, fill, dtype=dtype, device=self.dev)

        def p(t):
            return None if t is None else t.data_ptr()
        q = self._up(a["q"], np.float32)
        Q = len(a["q"])
        k = max(int(a.get("k", 0)), 0)
        any_, none_ = self._words(a.get("any_of")), self._words(a.get("none_of"))
        ins = [q, any_, none_]
        post = tuple
        if entry == "topk":
            outs = [full((Q, k), float("nan"), f64), full((Q, k), -7, i64)]
            h.score_topk_dev(p(q), Q, a["k"], p(outs[0]), p(outs[1]), s)
        elif entry == "rank":
            pq, pid = self._up(a["pair_q"], np.int32), self._up(a["pair_id"], np.int64)
            ins += [pq, pid]
            L = len(a["pair_q"])
            outs = [full((L,), -7, i64), full((L,), float("nan"), f64)]
            h.score_rank_dev(p(q), Q, p(pq), p(pid), L, None, p(outs[0]), p(outs[1]), s)
        elif entry in ("above", "count_above"):
            pq, thr = self._up(a["pair_q"], np.int32), self._up(a["thr"], np.float64)
            ins += [pq, thr]
            L = len(a["pair_q"])
            cap = a["cap"] if entry == "above" else 0
            outs = [full((L + 1,), -7, i64)] + ([full((cap,), -7, i64), full((cap,), float("nan"), f64)] if entry == "above" else [])
            h.score_above_dev(p(q), Q, p(pq), p(thr), L, cap, p(outs[0]), p(outs[1]) if cap else None, p(outs[2]) if cap else None, s)
            if entry == "count_above":
                post = lambda o: (np.diff(o[0]),)
            else:
                def post(o, cap=cap):
                    total = int(o[0][-1])
                    n = total if total <= cap else 0
                    assert (o[1][n:] == -7).all() and np.isnan(o[2][n:]).all(), "score_above_dev wrote behind the %d entries of its lists" % n
                    return o[0], o[1][:n], o[2][:n]
        elif entry == "filtered":
            ex = self._up(a.get("exclude"), np.int64)
            ins.append(ex)
            outs = [full((Q, k), float("nan"), f64), full((Q, k), -7, i64), full((Q,), -7, i32)]
            h.score_topk_filtered_dev(p(q), Q, a["k"], p(any_), p(none_), p(ex), 0 if ex is None else ex.shape[1], p(outs[0]), p(outs[1]), p(outs[2]), s)
        elif entry == "grouped":
            outs = [full((Q, k), float("nan"), f64), full((Q, k), -7, i64), full((Q, k), -7, i64), full((Q,), -7, i32)]
            h.score_topk_grouped_dev(p(q), Q, a["k"], p(any_), p(none_), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), s)
        elif entry == "after":
            cs = ci = None
            if a.get("after") is not None:
                cs, ci = self._up(a["after"][0], np.float64), self._up(a["after"][1], np.int64)
            ins += [cs, ci]
            outs = [full((Q, k), float("nan"), f64), full((Q, k), -7, i64), full((Q,), -7, i32)]
            h.score_topk_after_dev(p(q), Q, a["k"], p(cs), p(ci), p(any_), p(none_), p(outs[0]), p(outs[1]), p(outs[2]), s)
        else:
            raise ValueError(entry)
        return ins, outs, post

    def _queue(self, entry, a, own_stream):
        if not own_stream:
            return self._guard(self._enqueue, entry, a, 0)
        if self.stream is None:
            self.stream = self.torch.cuda.Stream(device=self.dev)
        with self.torch.cuda.stream(self.stream):              # uploads and pre-fills are ordered on the same stream
            return self._guard(self._enqueue, entry, a, self.stream.cuda_stream)

    def _finish(self):
        self.torch.cuda.synchronize()
        self._guard(self.h.synchronize)

    def call(self, entry, a, form):
        if form == "host":
            out = self._guard(self._host, entry, a)
            return tuple(np.asarray(x) for x in out)
        ins, outs, post = self._queue(entry, a, form == "queued")
        self._finish()
        return post(tuple(o.cpu().numpy() for o in outs))

    def queue_block(self, calls):
        """every call queued on one stream of its own (the handle's stream, sse_set_stream, is that stream for the duration),
        one synchronisation at the end"""
        if self.stream is None:
            self.stream = self.torch.cuda.Stream(device=self.dev)
        self.h.set_stream(self.stream.cuda_stream)
        try:
            pend = [self._queue(entry, a, True) for entry, a in calls]
            self._finish()
        finally:
            self.h.set_stream(0)
        return [post(tuple(o.cpu().numpy() for o in outs)) for ins, outs, post in pend]

    @staticmethod
    def _prefilled(o):
        """every element still holds what the device forms (and _raw_rank) fill outputs with: NaN or -7"""
        o = np.asarray(o)
        return bool(np.isnan(o).all()) if o.dtype.kind == "f" else bool((o == -7).all())

    def _raw_rank(self, a):
        """sse_score_rank on pre-filled host outputs (Handle.score_rank allocates its own and raises): (rc, message, outputs)"""
        import ctypes as C
        h = self.h
        q = np.ascontiguousarray(a["q"], np.float32)
        pq, pid = np.ascontiguousarray(a["pair_q"], np.int32), np.ascontiguousarray(a["pair_id"], np.int64)
        before, score = np.full(len(pq), -7, np.int64), np.full(len(pq), np.nan)

        def ptr(x):
            return x.ctypes.data_as(C.c_void_p)
        rc = h.lib.sse_score_rank(h._h, ptr(q), len(q), ptr(pq), ptr(pid), len(pq), None, ptr(before), ptr(score))
        return rc, h.lib.sse_last_error(h._h).decode(), (before, score)

    def call_refused(self, entry, a, form):
        """(message, None | the outputs, if any element no longer holds its pre-fill); the outputs if the call was served"""
        import sse_amd
        if form == "host":
            if entry == "rank" and a.get("pair_score") is None:
                rc, msg, outs = self._raw_rank(a)
                if rc == 0:
                    return outs
                return msg, (None if all(self._prefilled(o) for o in outs) else outs)
            return tuple(np.asarray(x) for x in self._guard(self._host, entry, a))
        ins, outs, post = self._queue(entry, a, form == "queued")       # (a host-side check raises here)
        self.torch.cuda.synchronize()
        try:
            self.h.synchronize()
        except sse_amd.SSEError as e:
            got = tuple(o.cpu().numpy() for o in outs)
            return str(e), (None if all(self._prefilled(o) for o in got) else got)
        return post(tuple(o.cpu().numpy() for o in outs))


_LIVE = []


@pytest.fixture(autouse=True)
def _close_long_lived_handles():
    yield
    while _LIVE:
        _LIVE.pop().close()


def _runner(name):
    _LIVE.append(GpuDriver())
    return SS.Runner(_LIVE[-1], fresh=GpuDriver, counters=NAMES, exempt=EXEMPT, name=name, out=print)


def _moved(r, counter):
    """the SCORESTATE lines of the calls that moved `counter`"""
    return [line for line in r.lines if counter.replace("score_", "") + "=" in line]


def test_replacement_chain():
    """Transition 1: A -> B -> A2 -> G -> Bx -> C -> Bu -> D64 -> D32 -> E -> F -> A, after every upload top-k on its three
    routes, rank, count / rows above, page 2.  A left-over of the larger index in idxp's padding rows or k-groups, idx_rm,
    idx64, idx_x3 or idx_base would show."""
    steps, where = SS.chain_script()
    r = _runner("chain").run(steps)
    b, bu = where[SS.CHAIN.index("B")], where[SS.CHAIN.index("Bu")]
    for i, j in zip(range(b[0], b[1] + 1), range(bu[0], bu[1] + 1)):      # the scalar pack of the unaligned pointer: B's bits
        assert SS.same_outputs(r.results[i - 1], r.results[j - 1]), (steps[i - 1], steps[j - 1])
    # D64 -> D32 moves the scores by what the oracle says (test_f64_rows_and_their_rounding_differ_on_the_device_as_in_the_oracle)
    from tests import topk_cases as TC
    bar = TC.score_bar(TC.BY_NAME["f64_rows"])
    d64, d32 = where[SS.CHAIN.index("D64")], where[SS.CHAIN.index("D32")]
    truth = []
    for name in ("D64", "D32"):
        o = SS.StateOracle()
        o.set_index(SS.index(name).rows, SS.index(name).how, 0)
        truth.append(o.call("topk", steps[d64[0] - 1].args)[0])
    want = truth[0] - truth[1]
    got = r.results[d64[0] - 1][0] - r.results[d32[0] - 1][0]
    assert np.abs(want).max() > 1e3 * bar and np.abs(got - want).max() <= 2 * bar
    print("SCORESTATE chain: %d steps, %d calls" % (len(r.done), sum(1 for s in r.done if s.kind == "call")))


def test_bf16_image_follows_the_index():
    """Transition 2: idxp16 is built lazily and must be rebuilt for A2, after score_bf16 0 -> 1 and for A again; the
    two-pass route (window narrowed around 9000 rows, Q = 1024) on both indexes.  A stale image leaves ids and scores exact
    and moves score_bf16_second_chance_queries / score_collect_queries / score_bruteforce_queries by about Q."""
    steps, _ = SS.bf16_script()
    r = _runner("bf16").run(steps)
    two_pass = _moved(r, "score_two_pass_calls")
    assert len(two_pass) == 2, two_pass                        # the route under test did run, once per form and index
    print("SCORESTATE bf16: %d steps, %d calls" % (len(r.done), sum(1 for s in r.done if s.kind == "call")))


def test_bound_follows_the_norm_of_the_index():
    """Transition 3: A2 -> A16 -> A2 on the planted construction (tests/test_score_state_host.py::test_band_preconditions): a
    stale idx_norm_max of either direction moves score_rank_band_rows / score_above_band_rows by 64 against the fresh handle."""
    r = _runner("norm").run(SS.norm_script())
    assert _moved(r, "score_rank_band_rows") and _moved(r, "score_above_band_rows")    # the bands are not empty: group 1 and the labels
    print("SCORESTATE norm: %d steps, %d calls" % (len(r.done), sum(1 for s in r.done if s.kind == "call")))


def test_tags_and_groups_live_and_die_with_the_index():
    """Transition 4."""
    steps, info = SS.tags_script()
    r = _runner("tags").run(steps)
    for group in info["same_as_topk"]:                       # calls without masks equal score_topk, bit for bit
        first = r.results[group[0] - 1]
        for j in group[1:]:
            assert SS.same_outputs(first[:2], r.results[j - 1][:2]) and (r.results[j - 1][2] == first[0].shape[1]).all(), steps[j - 1]
    assert _moved(r, "score_filtered_tiles_skipped")            # sorted tags: the tile skip did run
    print("SCORESTATE tags: %d steps, %d calls" % (len(r.done), sum(1 for s in r.done if s.kind == "call")))


def test_scratch_shared_between_entry_points():
    """Transition 5: every entry point in turn on A -- queued back to back on one stream with ONE synchronisation at the end
    (rank's 4097 pairs grow s_ccnt / s_cbuf / s_rk while the call before is in flight), then in the host form, then in the
    reverse order."""
    setup, calls, q = SS.scratch_script("queued")
    r = _runner("scratch").run(setup)
    r.step(SS.call("topk", "host", q=q, k=10))
    cursor = len(r.done)

    def order(form, rev=False):
        seq = [SS.call(c.entry, form, **c.args) if c is not None else SS.call("after", form, q=q, k=10, after=("page_after", cursor))
               for c in calls]
        return seq[::-1] if rev else seq
    r.block(order("queued"))
    r.run(order("host"))
    r.run(order("host", rev=True))
    r.block(order("queued", rev=True))
    print("SCORESTATE scratch: %d steps, %d calls" % (len(r.done), sum(1 for s in r.done if s.kind == "call")))


def test_refused_calls_leave_no_trace():
    """Transition 6: the good call after every refused one equals the fresh handle's, counters included; no pending device
    error surfaces in it."""
    nan, keep = np.full(3, np.nan), np.full(3, -7, np.int64)
    assert GpuDriver._prefilled(nan) and GpuDriver._prefilled(keep)        # what "the call wrote no output" is decided by
    assert not GpuDriver._prefilled(np.array([np.nan, 0.5])) and not GpuDriver._prefilled(np.array([-7, 0], np.int64))
    r = _runner("refused").run(SS.refused_script())
    print("SCORESTATE refused: %d steps, %d calls, %d refused" % (len(r.done), sum(1 for s in r.done if s.kind == "call"),
                                                                 sum(1 for s in r.done if s.kind == "refused")))


def test_refused_uploads_leave_no_trace():
    """Transition 6, uploads: on a float64 index with tags and keys, an upload of a refused shape through each of the three
    entry points; the calls after it equal the fresh handle's (the float64 rows still answer)."""
    r = _runner("refused_upload").run(SS.refused_upload_script())
    print("SCORESTATE refused_upload: %d steps, %d calls, %d refused" % (len(r.done), sum(1 for s in r.done if s.kind == "call"),
                                                                        sum(1 for s in r.done if s.kind == "refused")))


def test_two_handles_in_one_process():
    """Transition 7: X holds E (S = 620), Y holds G (S = 5), alternated call by call over every entry point (per-kernel
    attributes such as the dynamic-LDS limit are process-wide)."""
    x, y = SS.two_handles_script()
    runners = [_runner("X"), _runner("Y")]
    for who, st in SS.alternate(x, y):
        runners[who].step(st)
    print("SCORESTATE two handles: %d + %d steps" % (len(runners[0].done), len(runners[1].done)))


def test_encode_score_topk_between_the_others():
    """Transition 8: single-query encode_score_topk (the pinned mirror block, score_seq) between score_topk(Q = 700) and
    score_rank on an index of the scorer model's encoding size."""
    H = SS.index("H8")
    rng = np.random.RandomState(8)
    ids = [rng.randint(2, PARAMS["vocab_size"], size=(1, PARAMS["max_seq_length"])).astype(np.int32) for _ in range(3)]
    for t in ids:
        t[:, -1] = 1
    q700 = SS.queries("H8", 700, seed=8)
    pq = np.arange(10, dtype=np.int32)
    enc = [SS.call("encode_topk", ids=t, k=10) for t in ids]
    steps = [SS.set_index("H8"), enc[0], SS.call("topk", ("host", "dev"), q=q700, k=10), enc[1],
             SS.call("rank", ("host", "dev"), q=q700[:10], pair_q=pq, pair_id=np.arange(10, dtype=np.int64) * 29), enc[2], enc[0]]
    r = _runner("encode").run(steps)
    for j, st in enumerate(steps):
        if st.kind == "call" and st.entry == "encode_topk":     # the fused call returns score_topk's bits for its own encoding
            sc, rows, e = r.results[j]
            ws, wi = r.d.h.score_topk(e, 10)
            assert SS.bits_equal(sc, ws) and SS.bits_equal(rows, wi), st
            truth = SS.StateOracle()
            truth.set_index(H.rows, H.how, H.id_base)
            SS.against_truth("topk", (sc, rows), truth.call("topk", dict(q=e, k=10)), SS.score_tol(truth, e)[1])
    assert SS.same_outputs(r.results[1], r.results[-1])
    print("SCORESTATE encode: %d steps, %d calls" % (len(r.done), sum(1 for s in r.done if s.kind == "call")))
