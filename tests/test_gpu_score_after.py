"""sse_score_topk_after against the float64 oracle (DESIGN K6j; cases, reference and check in tests/after_cases.py, proven on the
CPU by tests/test_after_cases_host.py).

Every step of every case runs the host entry (Handle.score_topk_after) and the device entry (score_topk_after_dev, every stage
queued, outputs pre-filled with NaN / -7 / -7): the results are np.array_equal and check() holds them to the oracle -- ids and
counts exact, padding exact, no ineligible id, no row that is not after the cursor, no row twice, lower row first in an exact
tie, scores within max(1e-12, two float64 summation orders).  Cursor scores are midpoints the case proves safe or scores the
device returned in an earlier step.  The two score_after_* counters are read around each call.  Indexes of up to 1200 rows are
also held, bit for bit, to Handle.score_topk(q, k = N) of the same handle cut on the host.  One AFTERR line per case."""
import numpy as np
import pytest

from tests import after_cases as AC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

NAMES = ("score_after_collected_rows", "score_after_bruteforce_queries")


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _counters(h):
    return tuple(h.get_counter(n) for n in NAMES)


def _i64(a):
    """uint64 mask words as the int64 tensor of the same bits"""
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _host(h, q, k, after, any_, none_):
    return h.score_topk_after(q, k, after=after, any_of=any_, none_of=none_)


def _dev(h, q, k, after, any_, none_):
    import torch
    dev = torch.device("cuda:0")
    Q = q.shape[0]
    qd = torch.from_numpy(np.array(q, dtype=np.float32)).to(dev)
    ad = _i64(any_) if any_ is not None else None
    nd = _i64(none_) if none_ is not None else None
    csd = torch.from_numpy(np.array(after[0], dtype=np.float64)).to(dev) if after is not None else None
    cid = torch.from_numpy(np.array(after[1], dtype=np.int64)).to(dev) if after is not None else None
    out_s = torch.full((Q, k), float("nan"), dtype=torch.float64, device=dev)
    out_i = torch.full((Q, k), -7, dtype=torch.int64, device=dev)
    out_c = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    h.score_topk_after_dev(qd.data_ptr(), Q, k, csd.data_ptr() if csd is not None else None, cid.data_ptr() if cid is not None else None,
                           ad.data_ptr() if ad is not None else None, nd.data_ptr() if nd is not None else None,
                           out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr())
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy(), out_c.cpu().numpy()


def _set_index(h, case, keep):
    I = AC.inputs(case)
    t = I["t"]
    if case.upload == "dev":
        import torch
        d = torch.from_numpy(np.array(t, dtype=np.float32)).to("cuda:0")
        keep.append(d)
        h.index_set_dev(d.data_ptr(), t.shape[0], t.shape[1], id_base=case.id_base)
        torch.cuda.synchronize()
    else:
        assert t.dtype == (np.float64 if case.upload == "f64" else np.float32)
        h.index_upload(t, id_base=case.id_base)
    if I["tags"] is not None:
        h.index_set_tags(I["tags"])


def _cut_on_host(case, full_s, full_i, k, after):
    """Handle.score_topk(q, k = N) with the ineligible entries and the entries not after the cursor removed, cut to k, padded"""
    e = AC.eligible(case)
    ok = np.stack([e[qi, full_i[qi] - case.id_base] for qi in range(case.Q)])
    return AC.after_on_host(full_s, full_i, k, after, ok)


@pytest.mark.parametrize("case", AC.CASES, ids=repr)
def test_after_case(case):
    I = AC.inputs(case)
    assert AC.preconditions(case)
    h = _scorer()
    keep = []
    _set_index(h, case, keep)
    any_, none_ = I["any"], I["none"]
    full = h.score_topk(I["q"], case.N) if case.N <= 1200 else None
    known = [dict() for _ in range(case.Q)]
    worst, log, results = 0.0, [], []
    for st in AC.steps(case):
        after = AC.cursor_arrays(case, st, known)
        first = None
        for label, skip in case.variants:
            h.set_option("score_filtered_skip", skip)
            for entry in (_host, _dev):
                c0 = _counters(h)
                sc, ids, cnt = entry(h, I["q"], st.k, after, any_, none_)
                d = tuple(b - a for a, b in zip(c0, _counters(h)))
                log.append((st.label, label, entry.__name__, d))
                if first is None:
                    first = (sc, ids, cnt)
                else:
                    assert np.array_equal(ids, first[1]) and np.array_equal(sc, first[0]) and np.array_equal(cnt, first[2]), (case, st, label, entry.__name__)
                worst = max(worst, AC.check(case, st, sc, ids, cnt))
                assert d[1] == st.brute, (case, log)
                assert d[0] >= AC.collected_min(case, st), (case, log, AC.collected_min(case, st))
        h.set_option("score_filtered_skip", 1)
        if full is not None:                                  # the differential check
            ws, wi, wc = _cut_on_host(case, full[0], full[1], st.k, after)
            assert np.array_equal(first[1], wi) and np.array_equal(first[0], ws) and np.array_equal(first[2], wc), (case, st)
        AC.learn(known, *first)
        results.append(first)
    tol = AC.scales(case)[2]
    print("AFTERR %s Q %d N %d S %d base %d %s: worst |score - oracle| %.3e = %.3f tol (bar %.3e), (step, variant, entry, (collected, brute)) %s"
          % (case.name, case.Q, case.N, case.S, case.id_base, case.upload, worst, worst / tol, AC.score_bar(case), log))
    _extras(case, h, I, results, full)
    h.close()


def _extras(case, h, I, results, full):
    """what a case is held to beyond check(): the neighbours of the call on the same handle, bit for bit"""
    q = I["q"]
    steps = AC.steps(case)
    if case.first_page:
        k = steps[0].k
        ts, ti = h.score_topk(q, k)
        fs, fi, fc = h.score_topk_filtered(q, k)
        for sc, ids, cnt in results:                          # +inf and NULL
            assert np.array_equal(sc, ts) and np.array_equal(ids, ti) and (cnt == k).all()
            assert np.array_equal(sc, fs) and np.array_equal(ids, fi) and np.array_equal(cnt, fc)
    if case.name == "chain_k33":
        assert len(results) == 23 and (results[21][2] == 7).all() and not results[22][2].any()
        cat_s = np.concatenate([r[0][:, :int(r[2][0])] for r in results], axis=1)
        cat_i = np.concatenate([r[1][:, :int(r[2][0])] for r in results], axis=1)
        assert np.array_equal(cat_s, full[0]) and np.array_equal(cat_i, full[1])
    if case.name == "tags_one_of_eight":                      # page 2 by cursor = columns k .. 2k of the filtered call
        k = steps[0].k
        fs, fi, fc = h.score_topk_filtered(q, 2 * k, any_of=I["any"])
        assert (fc == 2 * k).all()
        assert np.array_equal(results[0][0], fs[:, :k]) and np.array_equal(results[0][1], fi[:, :k])
        assert np.array_equal(results[1][0], fs[:, k:]) and np.array_equal(results[1][1], fi[:, k:])
    if case.name == "k1024":                                  # rows 1025 .. 2048
        ts, ti = h.score_topk(q, 2048)
        assert np.array_equal(results[0][0], ts[:, :1024]) and np.array_equal(results[0][1], ti[:, :1024])
        assert np.array_equal(results[1][0], ts[:, 1024:]) and np.array_equal(results[1][1], ti[:, 1024:])
    if case.name == "overflow":                               # copies 2001 .. 2050 of the planted query
        p = case.base.planted[0]
        assert np.array_equal(results[1][1][p], case.id_base + I["group"][2000:2050])


def test_argument_errors_write_nothing_and_leave_the_handle_usable():
    import torch
    from sse_amd._lib import SSEError, _ptr
    case = AC.BY_NAME["tags_one_of_eight"]
    I = AC.inputs(case)
    st = AC.steps(case)[0]
    q = I["q"]
    Q = q.shape[0]
    h = _scorer()
    sc = np.full((Q, 1025), 123.0)
    ids = np.full((Q, 1025), -7, np.int64)
    cnt = np.full(Q, -7, np.int32)
    cs, ci = np.full(Q, np.inf), np.zeros(Q, np.int64)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.array(q)).to(dev)
    csd, cid, md = torch.from_numpy(cs).to(dev), torch.from_numpy(ci).to(dev), _i64(I["any"])
    d_sc = torch.full((Q, 1025), 123.0, dtype=torch.float64, device=dev)
    d_ids = torch.full((Q, 1025), -7, dtype=torch.int64, device=dev)
    d_cnt = torch.full((Q,), -7, dtype=torch.int32, device=dev)

    def both(k, match, score=True, id_=True, any_=False, none_=False):
        rc = h.lib.sse_score_topk_after(h._h, _ptr(q), Q, k, _ptr(cs) if score else None, _ptr(ci) if id_ else None,
                                        _ptr(I["any"]) if any_ else None, _ptr(I["any"]) if none_ else None, _ptr(sc), _ptr(ids), _ptr(cnt))
        assert rc != 0 and match in h.lib.sse_last_error(h._h).decode(), h.lib.sse_last_error(h._h)
        with pytest.raises(SSEError, match=match):
            h.score_topk_after_dev(qd.data_ptr(), Q, k, csd.data_ptr() if score else None, cid.data_ptr() if id_ else None,
                                   md.data_ptr() if any_ else None, md.data_ptr() if none_ else None,
                                   d_sc.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert (sc == 123.0).all() and (ids == -7).all() and (cnt == -7).all()
        assert bool((d_sc == 123.0).all()) and bool((d_ids == -7).all()) and bool((d_cnt == -7).all())

    def valid():
        if tagged:
            AC.check(case, st, *h.score_topk_after(q, st.k, after=(cs, ci), any_of=I["any"]))
        else:
            s1, i1, c1 = h.score_topk_after(q, st.k)
            ts, ti = h.score_topk(q, st.k)
            assert np.array_equal(s1, ts) and np.array_equal(i1, ti) and (c1 == st.k).all()

    tagged = False
    both(10, "no index")
    h.index_upload(I["t"])
    for k, match in ((0, "k = 0"), (-1, "k = -1"), (1025, "k = 1025")):
        both(k, match)
        valid()                                               # after each error the next valid call succeeds
    both(10, "after_id is missing", id_=False)
    valid()
    both(10, "after_score is missing", score=False)
    valid()
    both(10, "no tags", any_=True)
    valid()
    both(10, "no tags", none_=True)
    valid()
    h.index_set_tags(I["tags"])
    tagged = True
    valid()
    # Q == 0 succeeds and writes nothing
    s0, i0, c0 = h.score_topk_after(np.zeros((0, case.S), np.float32), 10)
    assert s0.shape == (0, 10) and i0.shape == (0, 10) and c0.shape == (0,)
    h.score_topk_after_dev(qd.data_ptr(), 0, 10, None, None, None, None, d_sc.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert bool((d_sc == 123.0).all()) and bool((d_cnt == -7).all())
    h.close()


def test_ranked_pages_and_ranked_rows():
    from sse_amd.sse_index import ranked_pages, ranked_rows
    case = AC.BY_NAME["chain_k33"]
    I = AC.inputs(case)
    q = I["q"]
    h = _scorer()
    h.index_upload(I["t"])
    fs, fi = h.score_topk(q, case.N)
    pages = list(ranked_pages(h, q, 300))
    assert [int(p[2][0]) for p in pages] == [300, 300, 100]
    assert np.array_equal(np.concatenate([p[0][:, :p[2][0]] for p in pages], axis=1), fs)
    assert np.array_equal(np.concatenate([p[1][:, :p[2][0]] for p in pages], axis=1), fi)
    for k_total, page in ((1, 1024), (450, 200), (700, 1024), (5000, 256)):
        rs, ri = ranked_rows(h, q, k_total, page=page)
        n = min(k_total, case.N)
        assert len(rs) == case.Q and all(a.shape == (n,) for a in rs)
        assert np.array_equal(np.stack(rs), fs[:, :n]) and np.array_equal(np.stack(ri), fi[:, :n])
    # tagged: every query's pages are its eligible rows in score_topk's order, lists of different lengths
    tcase = AC.BY_NAME["q33_nq4"]
    T = AC.inputs(tcase)
    h.index_upload(T["t"])
    h.index_set_tags(T["tags"])
    fs, fi = h.score_topk(T["q"], tcase.N)
    e = AC.eligible(tcase)
    got = [[] for _ in range(tcase.Q)]
    for sc, ids, cnt in ranked_pages(h, T["q"], 100, any_of=T["any"]):
        for qi in range(tcase.Q):
            got[qi].extend(zip(sc[qi, :cnt[qi]].tolist(), ids[qi, :cnt[qi]].tolist()))
    for qi in range(tcase.Q):
        keep = e[qi, fi[qi]]
        assert got[qi] == list(zip(fs[qi, keep].tolist(), fi[qi, keep].tolist())), qi
    h.close()
