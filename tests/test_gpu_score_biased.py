"""sse_score_topk_biased against the float64 oracle (DESIGN K6l; cases, reference and check in tests/biased_cases.py, proven on
the CPU by tests/test_biased_cases_host.py).

Every case runs the host entry (Handle.score_topk_biased), the device entry on the null stream (score_topk_biased_dev, outputs
pre-filled with NaN / -7 / -7) and the device entry queued twice back to back on a side stream: the results are np.array_equal
and check() holds them to the oracle -- ids and counts exact, padding exact, no ineligible id, no row twice, lower row first in
an exact tie, scores within the bar.  The two score_biased_* counters are read around each call.  The zero cases are also held,
byte for byte, to score_topk_filtered of the same handle.  One BIASEDR line per case."""
import numpy as np
import pytest

from tests import biased_cases as BC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

NAMES = ("score_biased_collected_rows", "score_biased_bruteforce_queries")


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _counters(h):
    return tuple(h.get_counter(n) for n in NAMES)


def _i64(a):
    """uint64 mask words as the int64 tensor of the same bits"""
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _host(h, q, k, w, any_, none_):
    return [h.score_topk_biased(q, k, weight=w, any_of=any_, none_of=none_)]


def _dev(h, q, k, w, any_, none_, side=False):
    import torch
    dev = torch.device("cuda:0")
    Q = q.shape[0]
    st = torch.cuda.Stream(device=dev) if side else torch.cuda.current_stream(dev)
    outs = []
    with torch.cuda.stream(st):
        qd = torch.from_numpy(np.array(q, dtype=np.float32)).to(dev)
        wd = torch.from_numpy(np.array(w, dtype=np.float32)).to(dev) if w is not None else None
        ad = _i64(any_) if any_ is not None else None
        nd = _i64(none_) if none_ is not None else None
        for _ in range(2 if side else 1):                     # (queued back to back: the second call reuses the first's scratch)
            out_s = torch.full((Q, k), float("nan"), dtype=torch.float64, device=dev)
            out_i = torch.full((Q, k), -7, dtype=torch.int64, device=dev)
            out_c = torch.full((Q,), -7, dtype=torch.int32, device=dev)
            h.score_topk_biased_dev(qd.data_ptr(), Q, k, wd.data_ptr() if wd is not None else None,
                                    ad.data_ptr() if ad is not None else None, nd.data_ptr() if nd is not None else None,
                                    out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr(), st.cuda_stream)
            outs.append((out_s, out_i, out_c))
    st.synchronize()
    torch.cuda.synchronize()
    return [tuple(o.cpu().numpy() for o in out) for out in outs]


def _dev_side(h, q, k, w, any_, none_):
    return _dev(h, q, k, w, any_, none_, side=True)


def _set_index(h, case, keep):
    import torch
    I = BC.inputs(case)
    t = I["t"]
    if case.upload == "dev":
        d = torch.from_numpy(np.array(t, dtype=np.float32)).to("cuda:0")
        keep.append(d)
        h.index_set_dev(d.data_ptr(), t.shape[0], t.shape[1], id_base=case.id_base)
        torch.cuda.synchronize()
    else:
        assert t.dtype == (np.float64 if case.upload == "f64" else np.float32)
        h.index_upload(t, id_base=case.id_base)
    if I["tags"] is not None:
        h.index_set_tags(I["tags"])
    if case.bias_entry == "dev":
        bd = torch.from_numpy(np.array(I["bias"])).to("cuda:0")
        h.index_set_bias_dev(bd.data_ptr(), case.N)
        torch.cuda.synchronize()                              # (the library has copied the values: bd may go)
    else:
        h.index_set_bias(I["bias"])


@pytest.mark.parametrize("case", BC.CASES, ids=repr)
def test_biased_case(case):
    I = BC.inputs(case)
    assert BC.preconditions(case)
    h = _scorer()
    keep = []
    _set_index(h, case, keep)
    first, worst, log = None, 0.0, []
    for entry in (_host, _dev, _dev_side):
        c0 = _counters(h)
        results = entry(h, I["q"], case.k, I["w"], I["any"], I["none"])
        d = tuple(b - a for a, b in zip(c0, _counters(h)))
        log.append((entry.__name__, d))
        for sc, ids, cnt in results:
            if first is None:
                first = (sc, ids, cnt)
            else:
                assert np.array_equal(ids, first[1]) and np.array_equal(sc, first[0]) and np.array_equal(cnt, first[2]), (case, entry.__name__)
            worst = max(worst, BC.check(case, sc, ids, cnt))
        assert d[1] == case.brute * len(results), (case, log)
        assert d[0] >= BC.collected_min(case) * len(results), (case, log, BC.collected_min(case))
    print("BIASEDR %s Q %d N %d S %d k %d base %d %s |w|bmax %.3g: worst |score - oracle| %.3e = %.3f tol (bar %.3e), (collected, brute) %s"
          % (case.name, case.Q, case.N, case.S, case.k, case.id_base, case.upload, BC.scales(case)[2], worst, worst / BC.scales(case)[3],
             BC.score_bar(case), log))
    if case.same_as_filtered:
        fs, fi, fc = h.score_topk_filtered(I["q"], case.k, any_of=I["any"], none_of=I["none"])
        assert first[0].tobytes() == fs.tobytes() and first[1].tobytes() == fi.tobytes() and first[2].tobytes() == fc.tobytes()
    h.close()


def test_refusals_carry_their_messages_write_nothing_and_leave_the_handle_usable():
    import torch
    from sse_amd._lib import SSEError, _ptr
    case = BC.BY_NAME["with_tags"]
    I = BC.inputs(case)
    q, bias = I["q"], I["bias"]
    Q = q.shape[0]
    h = _scorer()
    sc = np.full((Q, 1025), 123.0)
    ids = np.full((Q, 1025), -7, np.int64)
    cnt = np.full(Q, -7, np.int32)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.array(q)).to(dev)
    md = _i64(I["any"])
    d_sc = torch.full((Q, 1025), 123.0, dtype=torch.float64, device=dev)
    d_ids = torch.full((Q, 1025), -7, dtype=torch.int64, device=dev)
    d_cnt = torch.full((Q,), -7, dtype=torch.int32, device=dev)

    def both(k, masks, message):
        rc = h.lib.sse_score_topk_biased(h._h, _ptr(q), Q, k, None, _ptr(I["any"]) if masks else None, None, _ptr(sc), _ptr(ids), _ptr(cnt))
        assert rc != 0 and h.lib.sse_last_error(h._h).decode() == message
        with pytest.raises(SSEError) as ei:
            h.score_topk_biased_dev(qd.data_ptr(), Q, k, None, md.data_ptr() if masks else None, None,
                                    d_sc.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr())
        assert message in str(ei.value)
        torch.cuda.synchronize()
        assert (sc == 123.0).all() and (ids == -7).all() and (cnt == -7).all()
        assert bool((d_sc == 123.0).all()) and bool((d_ids == -7).all()) and bool((d_cnt == -7).all())

    both(10, False, "sse_score_topk_biased: no index uploaded")
    with pytest.raises(SSEError) as ei:
        h.index_set_bias(bias)
    assert "sse_index_set_bias: no index uploaded" in str(ei.value)
    h.index_upload(I["t"])
    both(10, False, "sse_score_topk_biased: the index has no bias (sse_index_set_bias)")
    h.index_set_bias(bias)
    both(10, True, "sse_score_topk_biased: tag masks given but the index has no tags (sse_index_set_tags)")
    both(0, False, "sse_score_topk_biased: k = 0 is not in [1, 1024]")
    both(1025, False, "sse_score_topk_biased: k = 1025 is not in [1, 1024]")
    h.index_set_tags(I["tags"])                               # after each error the next valid call succeeds
    want = h.score_topk_biased(q, case.k, any_of=I["any"])
    BC.check(case, *want)
    # wrong N, on both entries: the message, and the old bias is kept and still used
    for wrong in (bias[:-1], np.concatenate([bias, bias[:1]])):
        with pytest.raises(SSEError) as ei:
            h.index_set_bias(wrong)
        assert "sse_index_set_bias: %d values for an index of %d rows; the bias is unchanged" % (wrong.shape[0], case.N) in str(ei.value)
        wd = torch.from_numpy(np.array(wrong)).to(dev)
        with pytest.raises(SSEError, match="the bias is unchanged"):
            h.index_set_bias_dev(wd.data_ptr(), wrong.shape[0])
        torch.cuda.synchronize()
        for a, b in zip(h.score_topk_biased(q, case.k, any_of=I["any"]), want):
            assert np.array_equal(a, b)
    # a non-finite value in the host bias: refused after one pass, the old bias stays
    for pos, bad in ((0, np.nan), (case.N - 1, np.inf), (17, -np.inf)):
        nb = np.array(bias)
        nb[pos] = bad
        with pytest.raises(SSEError) as ei:
            h.index_set_bias(nb)
        assert "sse_index_set_bias: bias[%d] = " % pos in str(ei.value) and "is not finite; the bias is unchanged" in str(ei.value)
        for a, b in zip(h.score_topk_biased(q, case.k, any_of=I["any"]), want):
            assert np.array_equal(a, b)
    # Q == 0 succeeds and writes nothing
    s0, i0, c0 = h.score_topk_biased(np.zeros((0, case.S), np.float32), 10)
    assert s0.shape == (0, 10) and i0.shape == (0, 10) and c0.shape == (0,)
    h.score_topk_biased_dev(qd.data_ptr(), 0, 10, None, None, None, d_sc.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert bool((d_sc == 123.0).all()) and bool((d_cnt == -7).all())
    h.close()


def test_bias_lifecycle_and_the_state_a_biased_call_leaves():
    from sse_amd._lib import SSEError
    case = BC.BY_NAME["with_tags"]
    I = BC.inputs(case)
    q, any_, bias = I["q"], I["any"], I["bias"]
    h, other, fresh = _scorer(), _scorer(), _scorer()
    for x in (h, other, fresh):
        x.index_upload(I["t"])
        x.index_set_tags(I["tags"])
    other.index_set_bias(np.zeros(case.N, np.float32))        # a second handle with a bias of its own
    cursor = (np.full(case.Q, 0.3), np.zeros(case.Q, np.int64))

    def unbiased(x):
        return (x.score_topk(q, 12), x.score_topk(q, 40), x.score_topk_filtered(q, case.k, any_of=any_),
                x.score_topk_after(q, case.k, after=cursor, any_of=any_))

    before = unbiased(fresh)
    h.index_set_bias(bias)
    want = h.score_topk_biased(q, case.k, any_of=any_)
    BC.check(case, *want)
    # after a biased call the other calls of the handle return what a fresh handle returns, bit for bit
    for got, ref in zip(unbiased(h), before):
        for a, b in zip(got, ref):
            assert a.tobytes() == b.tobytes()
    # the second handle is unaffected: its zero bias gives the filtered call's rows
    for a, b in zip(other.score_topk_biased(q, case.k, any_of=any_), before[2]):
        assert a.tobytes() == b.tobytes()
    # setting tags or group keys does not touch the bias
    h.index_set_tags(I["tags"])
    h.index_set_groups(np.arange(case.N, dtype=np.int64) // 3)
    for a, b in zip(h.score_topk_biased(q, case.k, any_of=any_), want):
        assert a.tobytes() == b.tobytes()
    h.index_set_tags(None)
    with pytest.raises(SSEError, match="no tags"):
        h.score_topk_biased(q, case.k, any_of=any_)
    h.index_set_tags(I["tags"])
    # NULL clears
    h.index_set_bias(None)
    with pytest.raises(SSEError, match="has no bias"):
        h.score_topk_biased(q, case.k)
    h.index_set_bias(bias)
    for a, b in zip(h.score_topk_biased(q, case.k, any_of=any_), want):
        assert a.tobytes() == b.tobytes()
    # replacing the index clears the bias
    h.index_upload(I["t"])
    with pytest.raises(SSEError, match="has no bias"):
        h.score_topk_biased(q, case.k)
    h.index_set_tags(I["tags"])
    h.index_set_bias(bias)
    for a, b in zip(h.score_topk_biased(q, case.k, any_of=any_), want):
        assert a.tobytes() == b.tobytes()
    # a scalar weight is the weight of every query
    half = h.score_topk_biased(q, case.k, weight=0.5, any_of=any_)
    for a, b in zip(half, h.score_topk_biased(q, case.k, weight=np.full(case.Q, 0.5, np.float32), any_of=any_)):
        assert a.tobytes() == b.tobytes()
    assert not np.array_equal(half[0], want[0])
    for x in (h, other, fresh):
        x.close()


def test_csls_bias_gives_the_csls_ranking():
    from oracle import sse_oracle as O
    from sse_amd.sse_index import csls_bias
    from tests.test_biased_cases_host import csls_inputs, csls_reference
    tgt, src = csls_inputs()                                  # N = 400 targets (three hubs), M = 300 sources, S = 16
    assert tgt.shape == (400, 16) and src.shape == (300, 16)
    h = _scorer()
    b = csls_bias(h, tgt, src, k=10, block=128)
    assert b.dtype == np.float32 and np.abs(b.astype(np.float64) - csls_reference(tgt, src, 10)).max() <= 1e-6
    # the float64 CSLS order from the returned float32 bias
    s = O.scores_f64(src, tgt.astype(np.float64))
    csls = s + b.astype(np.float64)[None, :]
    ws, wi = O.topk(csls, 6)
    gap = ws[:, :-1] - ws[:, 1:]
    assert gap.min() > 1e-12, "the CSLS order of the inputs is not decided"
    assert (np.argmax(s, axis=1) != wi[:, 0]).any(), "the correction changes no query's best target"
    h.index_upload(tgt)                                       # csls_bias left the source rows in the handle
    h.index_set_bias(b)
    sc, ids, cnt = h.score_topk_biased(src, 5, weight=1.0)
    assert np.array_equal(ids, wi[:, :5]) and (cnt == 5).all() and np.abs(sc - ws[:, :5]).max() <= 1e-12
    plain, pid = h.score_topk(src, 1)
    assert (pid[:, 0] != ids[:, 0]).any()
    h.close()
