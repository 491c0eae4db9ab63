"""sse_score_topk_grouped against the float64 oracle (DESIGN K6h; cases, reference and check in tests/grouped_cases.py, proven on
the CPU by tests/test_grouped_cases_host.py).

Every case runs the host entry (Handle.score_topk_grouped) and the device entry (score_topk_grouped_dev, every stage queued,
outputs pre-filled with NaN / -7): the results are np.array_equal and check() holds them to the oracle -- ids, groups and counts
exact, padding exact, no group twice, every group by its best eligible row, lower row first in an exact tie, scores within
max(1e-12, two float64 summation orders).  The two score_grouped_* counters are read around each call.  Indexes of up to 1200
rows are also held, bit for bit, to Handle.score_topk(q, k = N) of the same handle collapsed on the host.  One GROUPED line per
case."""
import numpy as np
import pytest

from tests import grouped_cases as GC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

NAMES = ("score_grouped_collected_rows", "score_grouped_bruteforce_queries")


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _counters(h):
    return tuple(h.get_counter(n) for n in NAMES)


def _i64(a):
    """uint64 mask words as the int64 tensor of the same bits"""
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _host(h, q, k, any_, none_):
    return h.score_topk_grouped(q, k, any_of=any_, none_of=none_)


def _dev(h, q, k, any_, none_):
    import torch
    dev = torch.device("cuda:0")
    Q = q.shape[0]
    qd = torch.from_numpy(np.array(q, dtype=np.float32)).to(dev)
    ad = _i64(any_) if any_ is not None else None
    nd = _i64(none_) if none_ is not None else None
    out_s = torch.full((Q, k), float("nan"), dtype=torch.float64, device=dev)
    out_i = torch.full((Q, k), -7, dtype=torch.int64, device=dev)
    out_g = torch.full((Q, k), -7, dtype=torch.int64, device=dev)
    out_c = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    h.score_topk_grouped_dev(qd.data_ptr(), Q, k, ad.data_ptr() if ad is not None else None, nd.data_ptr() if nd is not None else None,
                             out_s.data_ptr(), out_i.data_ptr(), out_g.data_ptr(), out_c.data_ptr())
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy(), out_g.cpu().numpy(), out_c.cpu().numpy()


def _set_index(h, case, keep):
    I = GC.inputs(case)
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
    if case.group_entry == "dev":
        import torch
        gd = torch.from_numpy(np.array(I["groups"])).to("cuda:0")
        h.index_set_groups_dev(gd.data_ptr(), case.N)
        if I["tags"] is not None:
            td = _i64(I["tags"])
            h.index_set_tags_dev(td.data_ptr(), case.N)
        torch.cuda.synchronize()                              # (the library has copied the words: gd, td may go)
    else:
        h.index_set_groups(I["groups"])
        if I["tags"] is not None:
            h.index_set_tags(I["tags"])


def _collapse_on_host(case, full_s, full_i):
    """Handle.score_topk(q, k = N) with the ineligible columns and every later row of a group removed, cut to k, padded: what
    the call must return bit for bit"""
    e, g = GC.eligible(case), GC.inputs(case)["groups"]
    ws = np.full((case.Q, case.k), -np.inf)
    wi = np.full((case.Q, case.k), GC.PAD, np.int64)
    wg = np.full((case.Q, case.k), GC.PAD, np.int64)
    wc = np.zeros(case.Q, np.int32)
    for qi in range(case.Q):
        rows = full_i[qi] - case.id_base
        cols = np.flatnonzero(e[qi, rows])
        _, first = np.unique(g[rows[cols]], return_index=True)
        cols = cols[np.sort(first)][:case.k]
        c = cols.size
        ws[qi, :c], wi[qi, :c], wg[qi, :c], wc[qi] = full_s[qi, cols], full_i[qi, cols], g[rows[cols]], c
    return ws, wi, wg, wc


@pytest.mark.parametrize("case", GC.CASES, ids=repr)
def test_grouped_case(case):
    I = GC.inputs(case)
    assert GC.preconditions(case)
    h = _scorer()
    keep = []
    _set_index(h, case, keep)
    first, worst, log = None, 0.0, []
    for entry in (_host, _dev):
        c0 = _counters(h)
        got = entry(h, I["q"], case.k, I["any"], I["none"])
        d = tuple(b - a for a, b in zip(c0, _counters(h)))
        log.append((entry.__name__, d))
        if first is None:
            first = got
        else:
            for a, b in zip(got, first):
                assert np.array_equal(a, b), (case, entry.__name__)
    tol = GC.scales(case)[2]
    print("GROUPED %s Q %d N %d S %d k %d base %d %s: (collected, brute) %s, claimed brute %d collected >= %d"
          % (case.name, case.Q, case.N, case.S, case.k, case.id_base, case.upload, log, case.brute, GC.collected_min(case)))
    worst = GC.check(case, *first)
    print("GROUPED %s: worst |score - oracle| %.3e = %.3f tol (bar %.3e)" % (case.name, worst, worst / tol, GC.score_bar(case)))
    for _name, d in log:
        if case.brute != -1:
            assert d[1] == case.brute, (case, log)
        assert d[0] >= GC.collected_min(case), (case, log, GC.collected_min(case))
    if case.same_as_topk:
        ts, ti = h.score_topk(I["q"], case.k)
        assert np.array_equal(first[0], ts) and np.array_equal(first[1], ti) and (first[3] == case.k).all()
    if case.N <= 1200:                                        # the differential check
        fs, fi = h.score_topk(I["q"], case.N)
        for a, b in zip(first, _collapse_on_host(case, fs, fi)):
            assert np.array_equal(a, b), case
    h.close()


def test_group_key_lifecycle():
    case = GC.BY_NAME["random_groups_of_8"]
    I = GC.inputs(case)
    q, g = I["q"], I["groups"]
    h = _scorer()
    from sse_amd._lib import SSEError
    with pytest.raises(SSEError, match="no index"):
        h.index_set_groups(g)
    h.index_upload(I["t"])
    with pytest.raises(SSEError, match="no group keys"):
        h.score_topk_grouped(q, case.k)
    h.index_set_groups(g)
    want = h.score_topk_grouped(q, case.k)
    GC.check(case, *want)
    with pytest.raises(SSEError, match="unchanged"):          # wrong length: error, the old keys are kept
        h.index_set_groups(g[:-1])
    with pytest.raises(SSEError, match="unchanged"):
        h.index_set_groups(np.concatenate([g, g[:1]]))
    for a, b in zip(h.score_topk_grouped(q, case.k), want):
        assert np.array_equal(a, b)
    h.index_set_groups(None)                                  # NULL clears
    with pytest.raises(SSEError, match="no group keys"):
        h.score_topk_grouped(q, case.k)
    h.index_set_groups(g)
    tags = np.ones(case.N, np.uint64)
    h.index_set_tags(tags)                                    # tags and keys are independent: clearing one keeps the other
    h.index_set_groups(None)
    assert h.score_topk_filtered(q, case.k, any_of=np.ones(case.Q, np.uint64))[2].tolist() == [case.k] * case.Q
    h.index_set_groups(g)
    h.index_set_tags(None)
    for a, b in zip(h.score_topk_grouped(q, case.k), want):
        assert np.array_equal(a, b)
    h.index_upload(I["t"])                                    # a new index clears the keys
    with pytest.raises(SSEError, match="no group keys"):
        h.score_topk_grouped(q, case.k)
    h.index_set_groups(g)
    for a, b in zip(h.score_topk_grouped(q, case.k), want):
        assert np.array_equal(a, b)
    h.close()


def test_argument_errors_write_nothing_and_leave_the_handle_usable():
    import torch
    from sse_amd._lib import SSEError, _ptr
    case = GC.BY_NAME["random_groups_of_8"]
    I = GC.inputs(case)
    q = I["q"]
    Q = q.shape[0]
    h = _scorer()
    sc = np.full((Q, 1025), 123.0)
    ids = np.full((Q, 1025), -7, np.int64)
    grp = np.full((Q, 1025), -7, np.int64)
    cnt = np.full(Q, -7, np.int32)
    mask = np.ones(Q, np.uint64)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.array(q)).to(dev)
    md = torch.ones(Q, dtype=torch.int64, device=dev)
    d_sc = torch.full((Q, 1025), 123.0, dtype=torch.float64, device=dev)
    d_ids = torch.full((Q, 1025), -7, dtype=torch.int64, device=dev)
    d_grp = torch.full((Q, 1025), -7, dtype=torch.int64, device=dev)
    d_cnt = torch.full((Q,), -7, dtype=torch.int32, device=dev)

    def both(k, masks, match):
        rc = h.lib.sse_score_topk_grouped(h._h, _ptr(q), Q, k, _ptr(mask) if masks else None, None, _ptr(sc), _ptr(ids), _ptr(grp), _ptr(cnt))
        assert rc != 0 and match in h.lib.sse_last_error(h._h).decode()
        with pytest.raises(SSEError, match=match):
            h.score_topk_grouped_dev(qd.data_ptr(), Q, k, None, md.data_ptr() if masks else None,
                                     d_sc.data_ptr(), d_ids.data_ptr(), d_grp.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert (sc == 123.0).all() and (ids == -7).all() and (grp == -7).all() and (cnt == -7).all()
        assert bool((d_sc == 123.0).all()) and bool((d_ids == -7).all()) and bool((d_grp == -7).all()) and bool((d_cnt == -7).all())

    both(10, False, "no index")
    h.index_upload(I["t"])
    both(10, False, "no group keys")
    h.index_set_groups(I["groups"])
    both(0, False, "k = 0")
    both(1025, False, "k = 1025")
    both(-1, False, "k = -1")
    both(10, True, "no tags")
    GC.check(case, *h.score_topk_grouped(q, case.k))          # after each error the next valid call succeeds
    # Q == 0 succeeds and writes nothing
    s0, i0, g0, c0 = h.score_topk_grouped(np.zeros((0, case.S), np.float32), 10)
    assert s0.shape == (0, 10) and i0.shape == (0, 10) and g0.shape == (0, 10) and c0.shape == (0,)
    h.score_topk_grouped_dev(qd.data_ptr(), 0, 10, None, None, d_sc.data_ptr(), d_ids.data_ptr(), d_grp.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert bool((d_sc == 123.0).all()) and bool((d_cnt == -7).all())
    h.close()
