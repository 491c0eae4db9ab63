"""sse_score_topk_filtered against the float64 oracle (DESIGN K6g; cases, reference and check in tests/filtered_cases.py, proven
on the CPU by tests/test_filtered_cases_host.py).

Every case runs the host entry (Handle.score_topk_filtered) and the device entry (score_topk_filtered_dev, every stage queued,
outputs pre-filled with NaN / -7 / -7): the results are np.array_equal and check() holds them to the oracle -- ids and counts
exact, padding exact, no ineligible id, no row twice, lower row first in an exact tie, scores within max(1e-12, two float64
summation orders).  The three score_filtered_* counters are read around each call.  Indexes of up to 1200 rows are also held,
bit for bit, to Handle.score_topk(q, k = N) of the same handle filtered on the host.  One FILTERR line per case."""
import numpy as np
import pytest

from tests import filtered_cases as FC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

NAMES = ("score_filtered_collected_rows", "score_filtered_bruteforce_queries", "score_filtered_tiles_skipped")


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _counters(h):
    return tuple(h.get_counter(n) for n in NAMES)


def _i64(a):
    """uint64 mask words as the int64 tensor of the same bits"""
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _host(h, q, k, any_, none_, ex):
    return h.score_topk_filtered(q, k, any_of=any_, none_of=none_, exclude=ex)


def _dev(h, q, k, any_, none_, ex):
    import torch
    dev = torch.device("cuda:0")
    Q = q.shape[0]
    qd = torch.from_numpy(np.array(q, dtype=np.float32)).to(dev)
    ad = _i64(any_) if any_ is not None else None
    nd = _i64(none_) if none_ is not None else None
    ed = torch.from_numpy(np.array(ex, dtype=np.int64)).to(dev) if ex is not None else None
    out_s = torch.full((Q, k), float("nan"), dtype=torch.float64, device=dev)
    out_i = torch.full((Q, k), -7, dtype=torch.int64, device=dev)
    out_c = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    h.score_topk_filtered_dev(qd.data_ptr(), Q, k, ad.data_ptr() if ad is not None else None, nd.data_ptr() if nd is not None else None,
                              ed.data_ptr() if ed is not None else None, ex.shape[1] if ex is not None else 0,
                              out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr())
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy(), out_c.cpu().numpy()


def _set_index(h, case, keep):
    I = FC.inputs(case)
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
        if case.tag_entry == "dev":
            import torch
            td = _i64(I["tags"])
            h.index_set_tags_dev(td.data_ptr(), case.N)
            torch.cuda.synchronize()                          # (the library has copied the words: td may go)
        else:
            h.index_set_tags(I["tags"])


def _filter_on_host(case, full_s, full_i):
    """Handle.score_topk(q, k = N) with the ineligible columns removed, cut to k, padded: what the call must return bit for bit"""
    e = FC.eligible(case)
    ws = np.full((case.Q, case.k), -np.inf)
    wi = np.full((case.Q, case.k), FC.PAD_ID, np.int64)
    wc = np.zeros(case.Q, np.int32)
    for qi in range(case.Q):
        keep = e[qi, full_i[qi] - case.id_base]
        c = min(case.k, int(keep.sum()))
        ws[qi, :c], wi[qi, :c], wc[qi] = full_s[qi, keep][:c], full_i[qi, keep][:c], c
    return ws, wi, wc


@pytest.mark.parametrize("case", FC.CASES, ids=repr)
def test_filtered_case(case):
    I = FC.inputs(case)
    assert FC.preconditions(case)
    h = _scorer()
    keep = []
    _set_index(h, case, keep)
    first, worst, log = None, 0.0, []
    for label, skip, form, skipped in case.variants:
        h.set_option("score_filtered_skip", skip)
        any_, none_ = FC.masks(case, form)
        for entry in (_host, _dev):
            c0 = _counters(h)
            sc, ids, cnt = entry(h, I["q"], case.k, any_, none_, I["exclude"])
            d = tuple(b - a for a, b in zip(c0, _counters(h)))
            log.append((label, entry.__name__, d))
            if first is None:
                first = (sc, ids, cnt)
            else:
                assert np.array_equal(ids, first[1]) and np.array_equal(sc, first[0]) and np.array_equal(cnt, first[2]), (case, label, entry.__name__)
            worst = max(worst, FC.check(case, sc, ids, cnt))
            assert d[1] == case.brute, (case, log)
            assert d[0] >= FC.collected_min(case), (case, log, FC.collected_min(case))
            if skipped == "pos":
                assert d[2] > 0, (case, log)
            elif skipped == 0:
                assert d[2] == 0, (case, log)
    h.set_option("score_filtered_skip", 1)
    tol = FC.scales(case)[2]
    print("FILTERR %s Q %d N %d S %d k %d base %d %s: worst |score - oracle| %.3e = %.3f tol (bar %.3e), (collected, brute, skipped) %s"
          % (case.name, case.Q, case.N, case.S, case.k, case.id_base, case.upload, worst, worst / tol, FC.score_bar(case), log))
    if case.same_as_topk:
        ts, ti = h.score_topk(I["q"], case.k)
        assert np.array_equal(first[0], ts) and np.array_equal(first[1], ti) and (first[2] == case.k).all()
    if case.N <= 1200:                                        # the differential check
        fs, fi = h.score_topk(I["q"], case.N)
        ws, wi, wc = _filter_on_host(case, fs, fi)
        assert np.array_equal(first[1], wi) and np.array_equal(first[0], ws) and np.array_equal(first[2], wc), case
    h.close()


def test_tag_lifecycle():
    case = FC.BY_NAME["one_of_eight"]
    I = FC.inputs(case)
    q, any_ = I["q"], I["any"]
    h = _scorer()
    from sse_amd._lib import SSEError
    h.index_upload(I["t"])
    plain = h.score_topk_filtered(q, case.k)
    with pytest.raises(SSEError, match="no tags"):            # masks without tags
        h.score_topk_filtered(q, case.k, any_of=any_)
    with pytest.raises(SSEError, match="no tags"):
        h.score_topk_filtered(q, case.k, none_of=any_)
    for a, b in zip(h.score_topk_filtered(q, case.k), plain):  # ... and the next valid call succeeds
        assert np.array_equal(a, b)
    h.index_set_tags(I["tags"])
    want = h.score_topk_filtered(q, case.k, any_of=any_)
    FC.check(case, *want)
    with pytest.raises(SSEError, match="unchanged"):          # wrong length: error, the old tags are kept
        h.index_set_tags(I["tags"][:-1])
    with pytest.raises(SSEError, match="unchanged"):
        h.index_set_tags(np.concatenate([I["tags"], I["tags"][:1]]))
    for a, b in zip(h.score_topk_filtered(q, case.k, any_of=any_), want):
        assert np.array_equal(a, b)
    h.index_set_tags(None)                                    # NULL clears
    with pytest.raises(SSEError, match="no tags"):
        h.score_topk_filtered(q, case.k, any_of=any_)
    for a, b in zip(h.score_topk_filtered(q, case.k), plain):
        assert np.array_equal(a, b)
    h.index_set_tags(I["tags"])
    h.index_upload(I["t"])                                    # a new index clears the tags
    with pytest.raises(SSEError, match="no tags"):
        h.score_topk_filtered(q, case.k, any_of=any_)
    h.index_set_tags(I["tags"])
    for a, b in zip(h.score_topk_filtered(q, case.k, any_of=any_), want):
        assert np.array_equal(a, b)
    h.close()


def test_argument_errors_write_nothing_and_leave_the_handle_usable():
    import torch
    from sse_amd._lib import SSEError, _ptr
    case = FC.BY_NAME["one_of_eight"]
    I = FC.inputs(case)
    q = I["q"]
    Q = q.shape[0]
    h = _scorer()
    ex = np.zeros((Q, 65), np.int64)
    sc = np.full((Q, 1025), 123.0)
    ids = np.full((Q, 1025), -7, np.int64)
    cnt = np.full(Q, -7, np.int32)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.array(q)).to(dev)
    exd = torch.from_numpy(ex).to(dev)
    d_sc = torch.full((Q, 1025), 123.0, dtype=torch.float64, device=dev)
    d_ids = torch.full((Q, 1025), -7, dtype=torch.int64, device=dev)
    d_cnt = torch.full((Q,), -7, dtype=torch.int32, device=dev)

    def both(k, n_excl, match):
        rc = h.lib.sse_score_topk_filtered(h._h, _ptr(q), Q, k, None, None, _ptr(ex) if n_excl else None, n_excl, _ptr(sc), _ptr(ids), _ptr(cnt))
        assert rc != 0 and match in h.lib.sse_last_error(h._h).decode()
        with pytest.raises(SSEError, match=match):
            h.score_topk_filtered_dev(qd.data_ptr(), Q, k, None, None, exd.data_ptr() if n_excl else None, n_excl,
                                      d_sc.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert (sc == 123.0).all() and (ids == -7).all() and (cnt == -7).all()
        assert bool((d_sc == 123.0).all()) and bool((d_ids == -7).all()) and bool((d_cnt == -7).all())

    both(10, 0, "no index")
    h.index_upload(I["t"])
    both(0, 0, "k = 0")
    both(1025, 0, "k = 1025")
    both(-1, 0, "k = -1")
    both(10, 65, "n_excl = 65")
    both(10, -1, "n_excl = -1")
    h.index_set_tags(I["tags"])                               # after each error the next valid call succeeds
    FC.check(case, *h.score_topk_filtered(q, case.k, any_of=I["any"]))
    # Q == 0 succeeds and writes nothing
    s0, i0, c0 = h.score_topk_filtered(np.zeros((0, case.S), np.float32), 10)
    assert s0.shape == (0, 10) and i0.shape == (0, 10) and c0.shape == (0,)
    h.score_topk_filtered_dev(qd.data_ptr(), 0, 10, None, None, None, 0, d_sc.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert bool((d_sc == 123.0).all()) and bool((d_cnt == -7).all())
    h.close()


def test_hard_negatives():
    from oracle import sse_oracle as O
    from sse_amd.sse_index import hard_negatives
    rng = np.random.RandomState(321)
    q, t = FC.unit(rng, 200, 32), FC.unit(rng, 1000, 32)
    s = O.scores_f64(q, t.astype(np.float64))
    order = np.argsort(-s, axis=1, kind="stable")
    # positives: some of the best rows (the hard case) and a random one; between none and five per query
    positives = [sorted(set(order[i, :rng.randint(0, 5)].tolist() + ([int(rng.randint(1000))] if i % 3 else []))) for i in range(200)]
    h = _scorer()
    h.index_upload(t)
    n = 7
    ids, scores = hard_negatives(h, q, positives, n)
    assert ids.shape == (200, n) and scores.shape == (200, n)
    for i in range(200):
        assert not set(ids[i].tolist()) & set(positives[i])
        want = [r for r in order[i] if r not in positives[i]][:n]
        assert ids[i].tolist() == want
        assert np.abs(scores[i] - s[i, want]).max() <= 1e-12
    h.close()
