"""In-place updates and appends of the resident index (sse_index_update* / sse_index_append*, DESIGN K6n) against the one
contract: after any sequence of them the handle answers every scoring entry, bit for bit and score_* counter for counter, as a
FRESH handle given the final rows through the same upload entry and then set_tags / set_groups / set_bias -- and within the
bars of score_state_script.score_tol of the float64 oracle.  The runner, comparisons and oracle are tests/score_state_script's
(UpdateRunner of tests/index_update_script.py widens its vocabulary); GpuDriver is tests/test_gpu_score_state's."""
import numpy as np
import pytest

from tests import index_update_script as US
from tests import score_state_script as SS
from tests.test_gpu_score_state import NAMES, GpuDriver
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

T = 4                                                   # tokens per row of the drivers' models
TOKENS = np.random.RandomState(3).randint(2, 50, size=(6, T)).astype(np.int32)


class Driver(GpuDriver):
    """GpuDriver with a model whose encoding size is the index dimension (encode_topk on every index), the update / append /
    set_bias steps and the biased, lse and confusions entries in their three forms"""

    def __init__(self, S=8):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, S, T))
        self.h = self.m.handle
        self.rows = None
        self.stream = None

    def _enqueue(self, entry, a, s):
        if entry not in ("biased", "lse", "confusions"):
            return GpuDriver._enqueue(self, entry, a, s)
        T_, h = self.torch, self.h
        q = self._up(a["q"], np.float32)
        Q, k = len(a["q"]), int(a.get("k", 0))
        full = lambda shape, fill, dtype: T_.full(shape, fill, dtype=dtype, device=self.dev)
        nan = float("nan")
        if entry == "biased":
            outs = [full((Q, k), nan, T_.float64), full((Q, k), -7, T_.int64), full((Q,), -7, T_.int32)]
            h.score_topk_biased_dev(q.data_ptr(), Q, k, None, None, None, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), s)
            return [q], outs, tuple
        if entry == "lse":
            outs = [full((Q,), nan, T_.float64), full((Q,), -7, T_.int64), full((Q,), nan, T_.float64)]
            h.score_lse_dev(q.data_ptr(), Q, a["scale"], None, None, None, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), s)
            return [q], outs, tuple
        pos = self._up(a["positives"], np.int64)
        outs = [full((Q, k), nan, T_.float64), full((Q, k), -7, T_.int64), full((Q,), -7, T_.int32), full((Q,), nan, T_.float64),
                full((Q,), -7, T_.int64)]
        h.score_confusions_dev(q.data_ptr(), Q, k, pos.data_ptr(), pos.shape[1], float("inf"), outs[0].data_ptr(), outs[1].data_ptr(),
                               outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), s)
        return [q, pos], outs, tuple

    def set_bias(self, values):
        self._guard(self.h.index_set_bias, values)

    def _dev_cols(self, st):
        return self._words(st.tags), self._up(st.groups, np.int64), self._up(st.bias, np.float32)

    def update(self, st):
        if st.form == "host":
            return self._guard(self.h.index_update, st.ids, st.rows, st.tags, st.groups, st.bias)
        p = lambda t: None if t is None else t.data_ptr()
        ids, rows = self._up(st.ids, np.int64), self._up(st.rows, np.float32)
        t, g, b = self._dev_cols(st)
        self.torch.cuda.synchronize()
        self._guard(self.h.index_update_dev, p(ids), p(rows), len(st.ids), p(t), p(g), p(b))

    def append(self, st):
        if st.form == "host":
            return self._guard(self.h.index_append, st.rows, st.tags, st.groups, st.bias)
        p = lambda t: None if t is None else t.data_ptr()
        rows = self._up(st.rows, np.float32)
        t, g, b = self._dev_cols(st)
        self.torch.cuda.synchronize()
        return self._guard(self.h.index_append_dev, p(rows), len(st.rows), p(t), p(g), p(b))

    def _host(self, entry, a):
        h = self.h
        if entry == "biased":
            return h.score_topk_biased(a["q"], a["k"])
        if entry == "lse":
            return h.score_lse(a["q"], a["scale"])
        if entry == "confusions":
            return h.score_confusions(a["q"], a["k"], a["positives"])
        return GpuDriver._host(self, entry, a)


_LIVE = []


@pytest.fixture(autouse=True)
def _close_long_lived_handles():
    yield
    while _LIVE:
        _LIVE.pop().close()


def _runner(name, S=8):
    _LIVE.append(Driver(S))
    return US.UpdateRunner(_LIVE[-1], fresh=lambda: Driver(S), counters=NAMES, name=name, out=print)


def _battery(r, q, **kw):
    kw.setdefault("tokens", TOKENS)
    r.run(US.battery(r.state, q, len(r.done) + 1, **kw))


def _norm_bits_as_fresh(r):
    """idx_norm_max itself, read back: the bits a fresh handle forms for the final rows through the same upload entry (the
    per-row sums of the update must be the pack's own, on either pack path)"""
    f = r._build_fresh()
    try:
        want = f.h.index_norm_max()
    finally:
        f.close()
    got = r.d.h.index_norm_max()
    assert got.tobytes() == want.tobytes(), "idx_norm_max %r after the updates, %r on a fresh handle" % (got, want)


def _encode_topk(B):
    return SS.call("encode_topk", ids=np.random.RandomState(B).randint(2, 50, size=(B, T)).astype(np.int32), k=10)


def _begin(name, N, S, id_base=0, seed=1, cols=True, how="f32", Q=6):
    r = _runner(name, S)
    rows = US.unit(seed, N, S)
    if how == "f64":
        rows = rows.astype(np.float64) * (1.0 + 1e-9)
    r.step(US.start(name, rows, how, id_base))
    if cols:
        tags, groups, bias = US.columns(N, seed)
        r.run([SS.set_tags(tags), SS.set_groups(groups), US.set_bias(bias)])
    h = (Q + 1) // 2
    q = US.unit(seed + 50, h, S)
    q = np.concatenate([q, -q[:Q - h]])
    return r, q


def _new(r, ids, seed, scale=1.0):
    return (US.unit(seed, len(ids), r.state["rows"].shape[1]) * np.float32(scale)).astype(r.state["rows"].dtype)


def _cols(n, seed):
    return dict(zip(("tags", "groups", "bias"), US.columns(n, seed)))


@pytest.mark.parametrize("N,S,base", [(70, 50, 0), (571, 256, 1000)])
def test_update_cases(N, S, base):
    """M = 1, the tile seam (rows 31 and 32), first and last row, columns only, all rows; host and device forms"""
    r, q = _begin("upd%dx%d" % (N, S), N, S, base)
    for label, rows_, form in (("one", [5], "host"), ("seam", [31, 32], "dev"), ("ends", [0, N - 1], "host")):
        ids = np.array(rows_, np.int64) + base
        r.step(US.update(ids, _new(r, ids, 7 + len(r.done), scale=1.0 + 0.1 * len(ids)), form=form, label=label, **_cols(len(ids), 3 + len(r.done))))
        _norm_bits_as_fresh(r)
        _battery(r, q)
    ids = np.array([N - 1, 3, 33, 3], np.int64) + base            # any order, id 3 twice: the last entry wins
    r.step(US.update(ids, tags=[1, 2, 4, 7], bias=[0.5, -0.25, 0.0, 0.125], label="columns only"))
    assert r.state["tags"][3] == 7 and r.state["bias"][3] == np.float32(0.125)
    _battery(r, q)
    ids = np.arange(N, dtype=np.int64) + base
    r.step(US.update(ids, _new(r, ids, 99), form="dev", label="all rows"))
    _norm_bits_as_fresh(r)
    _battery(r, q)
    assert r.d.h.get_counter("index_update_calls") == 5 and r.d.h.get_counter("index_update_rows") == 1 + 2 + 2 + 3 + N


def test_replaced_top1_vanishes_and_equal_rows_tie_by_id():
    r, q = _begin("top1", 571, 256, 1000, cols=False)
    top = r.d.h.score_topk(q[:1], 1)[1][0, 0]
    rows = r.state["rows"]
    r.step(US.update([top], -rows[top - 1000][None, :], label="top-1 replaced by its negation"))
    assert top not in r.d.h.score_topk(q[:1], 17)[1]
    _battery(r, q)
    twin = int(r.d.h.score_topk(q[:1], 1)[1][0, 0])
    other = 1000 + (7 if twin != 1007 else 8)
    r.step(US.update([other], r.state["rows"][twin - 1000][None, :], form="dev", label="bit-equal to the top row"))
    sc, ids = r.d.h.score_topk(q[:1], 2)
    assert sc[0, 0] == sc[0, 1] and list(ids[0]) == sorted([twin, other])
    _battery(r, q)


def test_norm_bound_falls_and_rises():
    """The planted near-threshold rows of score_state_script.norm_script: a wrong idx_norm_max moves the band-row counters.
    Row 0 made 16 times as long (norm_max 16), then short again (norm_max must FALL back), then long once more."""
    q, t, groups, labels = SS.planted()
    r = _runner("norm", 64)
    r.step(US.start("A2", t, "f32", 0))
    ids = np.array(labels, np.int64)
    pq = np.arange(SS.PLANT_Q, dtype=np.int32)
    calls = [SS.call("rank", ("host", "dev"), q=q, pair_q=pq, pair_id=ids)]
    r.run(calls)
    for scale, form in ((16.0, "host"), (1.0, "dev"), (16.0, "dev")):
        r.step(US.update([0], (t[:1] * np.float32(scale)), form=form, label="row 0 x %g" % scale))
        _norm_bits_as_fresh(r)
        r.run(calls)
    moved = [line for line in r.lines if "rank_band_rows=" in line]
    assert moved, "no call needed float64 for a band row: the planted rows are not near the threshold any more"


@pytest.mark.parametrize("S", [50, 256])
def test_append_cases(S):
    """within the tail tile, filling it exactly, into new tiles, past capacity twice"""
    N = 70 if S == 50 else 571
    base = 0 if S == 50 else 1000
    r, q = _begin("app%d" % S, N, S, base)
    tail = 32 - N % 32
    for label, M, form in (("inside the tail tile", 3, "host"), ("filling it", tail - 3, "dev"), ("new tiles", 40, "host"), ("doubling", 2 * N, "dev")):
        n0 = len(r.state["rows"])
        first = r.d.h.index_base + r.d.h.index_rows
        r.step(US.append(US.unit(11 + n0, M, S), form=form, label=label, **_cols(M, n0)))
        assert first == base + n0 and r.d.h.index_rows == n0 + M
        _norm_bits_as_fresh(r)
        _battery(r, q)
    assert r.d.h.get_counter("index_grow_copies") == 2
    assert r.d.h.get_counter("index_append_rows") == 3 + tail - 3 + 40 + 2 * N


def test_append_past_the_small_index_scorer():
    """1000 -> 1100 rows with Q >= 1024 queries: idx_x3 and the small-index route stop being used, as on a fresh handle"""
    r, _ = _begin("x3", 1000, 64, 0, cols=False)
    q = SS._unit(77, 1024, 64)
    same = [SS.call("topk", ("host", "dev"), q=q, k=10), _encode_topk(1024)]
    r.run(same)
    r.step(US.update([5, 999], US.unit(5, 2, 64), label="two rows, idx_x3 live"))
    r.run(same)
    r.step(US.append(US.unit(6, 100, 64), form="dev", label="past 1024"))
    r.run(same)


def test_bf16_image_patched_not_rebuilt():
    """N = 8200: a bf16 call builds idxp16, 3 scattered rows are replaced and 40 appended, the bf16 route again; then the
    two-pass route with its window narrowed around the index (as score_state_script.bf16_script does)"""
    r, _ = _begin("bf16", 8200, 64, 0, cols=False)
    qa = SS._unit(78, 129, 64)
    qm = SS._unit(79, 1024, 64)
    same = [SS.call("topk", ("host", "dev"), q=qa, k=10), _encode_topk(129)]
    r.run([SS.set_option("score_bf16", 1)] + same)
    r.step(US.update([0, 4111, 8199], US.unit(8, 3, 64), form="dev", label="three scattered rows"))
    r.run(same)
    r.step(US.append(US.unit(9, 40, 64), label="40 rows"))
    r.run(same)
    r.run([SS.set_option("score_two_pass_min_rows", 8000), SS.set_option("score_two_pass_rows", 9000), SS.call("topk", ("host", "dev"), q=qm, k=10)])
    assert r.d.h.get_counter("score_two_pass_calls") >= 1


def test_two_pass_route_after_updates():
    """N = 49 160, S = 64, Q = 1024: the two-pass route of mid-size indexes on a patched idxp16"""
    r, _ = _begin("twopass", 49160, 64, 0, cols=False)
    q = SS._unit(80, 1024, 64)
    same = [SS.call("topk", ("host",), q=q, k=10)]
    r.run(same)                                                       # (builds idxp16)
    c0 = r.d.h.get_counter("score_two_pass_calls")
    assert c0 >= 1
    r.step(US.update([1, 24000, 49159], US.unit(13, 3, 64), form="dev", label="three scattered rows"))
    r.step(US.append(US.unit(14, 40, 64), form="dev", label="40 rows"))
    r.run(same)
    assert r.d.h.get_counter("score_two_pass_calls") > c0


def test_row_major_copy_dropped_past_64_mib():
    """N = 65 500 x 256 floats is 63.96 MiB: 100 more rows take it past the 64 MiB a handle keeps row-major"""
    r, q = _begin("rm", 65500, 256, 0, cols=False, Q=4)
    same = [SS.call("topk", ("host",), q=q, k=10)]
    r.run(same)
    r.step(US.append(US.unit(12, 100, 256), form="dev", label="past 64 MiB"))
    r.run(same)


def test_f64_forms():
    r, q = _begin("f64", 70, 48, 3, how="f64")
    ids = np.array([0, 31, 32, 69], np.int64) + 3
    r.step(US.update(ids, _new(r, ids, 21) * (1.0 + 1e-9), label="f64 rows"))
    _battery(r, q)
    r.step(US.append(US.unit(22, 30, 48).astype(np.float64) * (1.0 - 1e-9), label="f64 append", **_cols(30, 5)))
    _battery(r, q)
    r.step(SS.refused(US.update(ids, _new(r, ids, 23).astype(np.float32), label="f32 on f64"), "float64 rows"))
    _battery(r, q)


def test_refusals_change_nothing():
    import sse_amd
    d = Driver()
    _LIVE.append(d)
    with pytest.raises(sse_amd.SSEError, match="no index uploaded"):
        d.h.index_update([0], np.zeros((1, 8), np.float32))
    with pytest.raises(sse_amd.SSEError, match="no index uploaded"):
        d.h.index_append(np.zeros((1, 8), np.float32))
    r, q = _begin("refuse", 70, 50, 10)
    S = 50
    one = US.unit(1, 1, S)
    bad = [
        (US.update([9], one), "outside the index"),
        (US.update([80], one), "outside the index"),
        (US.update([11, 11], np.repeat(one, 2, 0), form="dev"), "strictly increasing"),
        (US.update([12, 11], np.repeat(one, 2, 0), form="dev"), "strictly increasing"),
        (US.update([11, 500], np.repeat(one, 2, 0), form="dev"), "outside the index|strictly increasing"),
        (US.update([11], one.astype(np.float64)), "no float64 rows"),
        (US.update([11], bias=[np.inf]), "not finite"),
        (US.append(one, tags=[1], groups=[1]), "exactly when"),
        (US.append(one), "exactly when"),
        (US.append(one, tags=[1], groups=[1], bias=[np.nan]), "not finite"),
    ]
    for st, regex in bad:
        r.step(SS.refused(st, regex))
    # at the C ABI, where the wrapper cannot get in the way: N + M beyond the int32 row limit (refused before an operand is
    # read: the buffers hold one row), rows == NULL on an append, ids == NULL on an update; host and device forms
    import ctypes as C
    import torch
    h, lib = r.d.h, r.d.h.lib
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    t1, g1, b1 = np.ones(1, np.uint64), np.ones(1, np.int64), np.zeros(1, np.float32)
    i1 = np.array([11], np.int64)
    dv = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to("cuda:0")
    dr, dt, dg, db, di = dv(one.reshape(-1)), dv(t1), dv(g1), dv(b1), dv(i1)
    D = lambda x: C.c_void_p(x.data_ptr())
    torch.cuda.synchronize()
    HUGE = 2147483000
    for fn, regex in (
            (lambda: lib.sse_index_append(h._h, P(one), HUGE, P(t1), P(g1), P(b1)), "too large for int32 row ids"),
            (lambda: lib.sse_index_append_dev(h._h, D(dr), HUGE, D(dt), D(dg), D(db), None), "too large for int32 row ids"),
            (lambda: lib.sse_index_append(h._h, None, 1, P(t1), P(g1), P(b1)), "rows must not be NULL"),
            (lambda: lib.sse_index_append_dev(h._h, None, 1, D(dt), D(dg), D(db), None), "rows must not be NULL"),
            (lambda: lib.sse_index_update(h._h, None, P(one), 1, None, None, None), "ids must not be NULL"),
            (lambda: lib.sse_index_update_dev(h._h, None, D(dr), 1, None, None, None, None), "ids must not be NULL"),
            (lambda: lib.sse_index_update(h._h, P(i1), P(one), -1, None, None, None), "M = -1")):
        rc = fn()
        assert rc != 0 and __import__("re").search(regex, lib.sse_last_error(h._h).decode()), (rc, regex, lib.sse_last_error(h._h))
    assert h.index_shape() == (70, 50, 10)
    ids = np.zeros(0, np.int64)
    r.d.h.index_update(ids, np.zeros((0, S), np.float32))           # M == 0 succeeds and changes nothing
    _battery(r, q)
    r.run([SS.set_tags(None)])
    r.step(SS.refused(US.update([11], tags=[1]), "not set on the resident index"))
    r.step(SS.refused(US.update([11]), "nothing to update"))
    _battery(r, q)
    assert r.d.h.get_counter("index_update_calls") == 0 and r.d.h.get_counter("index_append_rows") == 0


def test_two_handles_and_upload_after_updates():
    a, q = _begin("ha", 70, 50, 0)
    b, _ = _begin("hb", 70, 50, 0)
    a.step(US.update([3, 40], US.unit(31, 2, 50), label="on a"))
    b.step(US.append(US.unit(32, 5, 50), label="on b", **_cols(5, 9)))
    _battery(a, q)
    _battery(b, q)
    a.step(US.start("again", US.unit(33, 40, 50), "f32", 0))        # an upload forgets the updates, the columns and the norms
    _battery(a, q)
    a.step(US.update([39], US.unit(34, 1, 50) * np.float32(3.0), form="dev", label="after the new upload"))
    _battery(a, q)


def test_ranker_update_targets():
    """Ranker.update_targets, then a rank(): the new rows answer, exactly as a ranker that was given the final encodings"""
    from tests.test_gpu_serving_after import N, T, _ranker
    r = _ranker()
    fresh = _ranker()
    try:
        h = r.model.handle
        rng = np.random.RandomState(8)
        toks = rng.randint(2, 50, size=(2, T)).astype(np.int32)
        query = rng.randint(2, 50, size=(1, T)).astype(np.int32)
        before = dict((t[1], t[0]) for t in r.rank(query, N, True)[0])
        r.update_targets([17, 250], toks)
        new = h.encode(1, toks, True).astype(np.float64)
        assert SS.bits_equal(r._encodings[[17, 250]], new)
        got = r.rank(query, N, True)[0]
        fresh.model.handle.index_upload(r._encodings)
        fresh._index_gen, fresh._encodings = fresh.model.handle.index_gen, r._encodings
        assert got == fresh.rank(query, N, True)[0]
        after = dict((t[1], t[0]) for t in got)
        q64 = h.encode(0, query, True).astype(np.float64)[0]
        for i, row in ((17, new[0]), (250, new[1])):
            assert abs(after["id%d" % i] - float(q64.dot(row))) < 1e-12 and after["id%d" % i] != before["id%d" % i]
        assert h.get_counter("index_update_rows") == 2
    finally:
        r.model.handle.close()
        fresh.model.handle.close()


def test_python_surface():
    """refresh_rows against encode + index_update (and encode_topk on the refreshed index); ShardedIndex.update_rows on two
    logical shards against the unsharded handle"""
    from sse_amd import sharded, sse_index
    r, q = _begin("py", 300, 8, 0, cols=False)
    m = r.d.m
    rng = np.random.RandomState(4)
    toks = rng.randint(2, 50, size=(4, 4)).astype(np.int32)
    ids = np.array([299, 7, 100, 7], np.int64)                        # id 7 twice: the last token row wins
    assert sse_index.refresh_rows(m, m.handle, ids, toks) == 3
    enc = m.handle.encode(1, toks)
    r.state["rows"][ids] = enc                                        # what encode + index_update leave
    r._sync_truth()
    _battery(r, q)
    r.run([SS.call("encode_topk", ids=toks, k=3)])
    # two logical shards, each on a handle of its own, against one handle holding everything
    rows = r.state["rows"]
    new = US.unit(41, 3, 8)
    uid = np.array([5, 149, 150], np.int64)
    parts = []
    for rank in range(2):
        d = Driver()
        _LIVE.append(d)
        sh = sharded.ShardedIndex(d.h, rank, 2, 300)
        d.h.index_upload(rows[sh.start:sh.end], id_base=sh.start)
        assert sh.update_rows(uid, new) == (2 if rank == 0 else 1)
        parts.append(d.h.score_topk(q, 5))
    r.step(US.update(uid, new, label="unsharded"))
    sc, ix = r.d.h.score_topk(q, 5)
    both_s, both_i = np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
    order = np.lexsort((both_i, -both_s), axis=1)[:, :5]
    assert SS.bits_equal(np.take_along_axis(both_i, order, 1), ix) and SS.bits_equal(np.take_along_axis(both_s, order, 1), sc)
