"""sse_score_lse against the float64 restatement (DESIGN K6m; cases, reference and check in tests/lse_cases.py, proven on the
CPU by tests/test_lse_cases_host.py).

Every case runs the host entry (Handle.score_lse), the device entry on the null stream (score_lse_dev, outputs pre-filled with
NaN / -7 / NaN) and the device entry queued twice back to back on a side stream: the results are np.array_equal and check()
holds them to the reference -- counts exact, -inf exactly on the empty sets, no NaN, |lse - reference| <= bound, and the bound
within 2^-14 of the dot part.  One LSER line per case."""
import numpy as np
import pytest

from tests import lse_cases as LC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

NAMES = ("score_lse_calls", "score_lse_tiles_skipped")


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _counters(h):
    return tuple(h.get_counter(n) for n in NAMES)


def _i64(a):
    """uint64 mask words as the int64 tensor of the same bits"""
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _host(h, q, scale, w, any_, none_):
    return [h.score_lse(q, scale, weight=w, any_of=any_, none_of=none_)]


def _dev(h, q, scale, w, any_, none_, side=False):
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
            out_l = torch.full((Q,), float("nan"), dtype=torch.float64, device=dev)
            out_c = torch.full((Q,), -7, dtype=torch.int64, device=dev)
            out_b = torch.full((Q,), float("nan"), dtype=torch.float64, device=dev)
            h.score_lse_dev(qd.data_ptr(), Q, scale, wd.data_ptr() if wd is not None else None,
                            ad.data_ptr() if ad is not None else None, nd.data_ptr() if nd is not None else None,
                            out_l.data_ptr(), out_c.data_ptr(), out_b.data_ptr(), st.cuda_stream)
            outs.append((out_l, out_c, out_b))
    st.synchronize()
    torch.cuda.synchronize()
    return [tuple(o.cpu().numpy() for o in out) for out in outs]


def _dev_side(h, q, scale, w, any_, none_):
    return _dev(h, q, scale, w, any_, none_, side=True)


def _set_index(h, case, keep):
    import torch
    I = LC.inputs(case)
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
    if I["bias"] is not None:
        h.index_set_bias(I["bias"])


def _run(case):
    """the case through the three entries on a fresh handle: (the first result, worst share of the bound, worst bound - d_q, counter log)"""
    I = LC.inputs(case)
    h = _scorer()
    keep = []
    _set_index(h, case, keep)
    first, used, over, log = None, 0.0, 0.0, []
    for entry in (_host, _dev, _dev_side):
        c0 = _counters(h)
        results = entry(h, I["q"], case.scale, I["w"], I["any"], I["none"])
        d = tuple(b - a for a, b in zip(c0, _counters(h)))
        log.append((entry.__name__, d))
        assert d[0] == len(results), (case, log)
        for lse, cnt, bnd in results:
            if first is None:
                first = (lse, cnt, bnd)
            else:
                assert np.array_equal(lse, first[0]) and np.array_equal(cnt, first[1]) and np.array_equal(bnd, first[2]), (case, entry.__name__)
            u, o = LC.check(case, lse, cnt, bnd)
            used, over = max(used, u), max(over, o)
    skipped = [d[1] // max(d[0], 1) for _, d in log]
    assert len(set(skipped)) == 1, (case, log)                # every call skips the same tiles
    if case.name == "tags_skip":
        assert skipped[0] > 0, "no tile was skipped"
    if LC.inputs(case)["tags"] is None:
        assert skipped[0] == 0
    h.close()
    return first, used, over, log


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_lse_case(case):
    first, used, over, log = _run(case)
    nsplit = str(LC.nsplit_of(case.Q, case.N)) if case.Q <= 32 else "-"
    if case.nsplit is not None:
        assert LC.nsplit_of(case.Q, case.N) == case.nsplit
    print("LSER %s Q %d N %d S %d scale %g base %d %s NSPLIT %s: worst |lse - ref| = %.4f of the bound, bound - d_q <= %.3e (budget %.3e), %s"
          % (case.name, case.Q, case.N, case.S, case.scale, case.id_base, case.upload, nsplit, used, over, LC.REST, log))


def test_ascending_and_descending_order_agree_within_the_bound():
    a, d = LC.BY_NAME["ascending"], LC.BY_NAME["descending"]
    ra, rd = _run(a)[0], _run(d)[0]
    assert np.array_equal(ra[1], rd[1])
    assert (np.abs(ra[0] - rd[0]) <= ra[2] + rd[2]).all()
    print("LSER ascending vs descending: |difference| %.3e, bound %.3e" % (np.abs(ra[0] - rd[0]).max(), ra[2].max()))


@pytest.mark.parametrize("name", ["bias_mixed", "bias_and_tags", "tags_mixed"])
def test_probabilities_of_the_whole_ranked_list_sum_to_one(name):
    """softmax_probs of score_topk_biased (k = N) -- of score_topk_filtered for the case without a bias -- and this call's lse"""
    from sse_amd.sse_index import softmax_probs
    case = LC.BY_NAME[name]
    assert case.N <= 1024
    I = LC.inputs(case)
    h = _scorer()
    _set_index(h, case, [])
    lse, cnt, bound = h.score_lse(I["q"], case.scale, weight=I["w"], any_of=I["any"], none_of=I["none"])
    LC.check(case, lse, cnt, bound)
    if I["w"] is not None:
        sc, _, c = h.score_topk_biased(I["q"], case.N, weight=I["w"], any_of=I["any"], none_of=I["none"])
    else:
        sc, _, c = h.score_topk_filtered(I["q"], case.N, any_of=I["any"], none_of=I["none"])
    assert np.array_equal(c.astype(np.int64), cnt)
    p = softmax_probs(sc, lse, case.scale)
    assert not np.isnan(p).any() and (p[np.arange(case.N)[None, :] >= cnt[:, None]] == 0).all()
    total = p.sum(1)
    live = cnt > 0
    assert (total[~live] == 0).all()
    assert (np.abs(total[live] - 1.0) <= np.expm1(bound[live])).all(), (total, bound)
    print("LSER %s: |sum of P - 1| <= %.3e, expm1(bound) >= %.3e" % (name, np.abs(total[live] - 1.0).max(), np.expm1(bound[live]).min()))
    h.close()


def test_state_a_long_lived_handle_keeps():
    """after another index, after the tags were cleared and after the bias was cleared a call equals the call on a fresh handle bit
    for bit, and the score_lse_* counters move by the same amounts"""
    from sse_amd._lib import SSEError
    case, other = LC.BY_NAME["bias_and_tags"], LC.BY_NAME["tags_skip"]
    I, J = LC.inputs(case), LC.inputs(other)

    def calls(x, tags, bias):
        c0 = _counters(x)
        out = [x.score_lse(I["q"], case.scale)]
        if tags:
            out.append(x.score_lse(I["q"], case.scale, any_of=I["any"], none_of=I["none"]))
        if bias:
            out.append(x.score_lse(I["q"], case.scale, weight=I["w"]))
        if tags and bias:
            out.append(x.score_lse(I["q"], case.scale, weight=I["w"], any_of=I["any"], none_of=I["none"]))
        return out, tuple(b - a for a, b in zip(c0, _counters(x)))

    def same(a, b):
        assert a[1] == b[1], (a[1], b[1])
        assert len(a[0]) == len(b[0])
        for x, y in zip(a[0], b[0]):
            for u, v in zip(x, y):
                assert u.tobytes() == v.tobytes()

    def fresh(tags, bias):
        f = _scorer()
        f.index_upload(I["t"])
        if tags:
            f.index_set_tags(I["tags"])
        if bias:
            f.index_set_bias(I["bias"])
        out = calls(f, tags, bias)
        f.close()
        return out

    h = _scorer()
    # another index first, with its own tags, scored with masks (tiles skipped) and Q of another size
    _set_index(h, other, [])
    LC.check(other, *h.score_lse(J["q"], other.scale, any_of=J["any"]))
    h.index_upload(I["t"])                                    # a new index clears tags and bias
    with pytest.raises(SSEError, match="no tags"):
        h.score_lse(I["q"], case.scale, any_of=I["any"])
    with pytest.raises(SSEError, match="no bias"):
        h.score_lse(I["q"], case.scale, weight=I["w"])
    same(calls(h, False, False), fresh(False, False))
    h.index_set_tags(I["tags"])
    h.index_set_bias(I["bias"])
    full = calls(h, True, True)
    same(full, fresh(True, True))
    LC.check(case, *full[0][3])
    h.index_set_tags(None)
    with pytest.raises(SSEError, match="no tags"):
        h.score_lse(I["q"], case.scale, none_of=I["none"])
    same(calls(h, False, True), fresh(False, True))
    h.index_set_tags(I["tags"])
    h.index_set_bias(None)
    with pytest.raises(SSEError, match="no bias"):
        h.score_lse(I["q"], case.scale, weight=I["w"])
    same(calls(h, True, False), fresh(True, False))
    # the other scoring calls of the handle are what a fresh handle returns
    f = _scorer()
    f.index_upload(I["t"])
    f.index_set_tags(I["tags"])
    for a, b in zip(h.score_topk_filtered(I["q"], 10, any_of=I["any"]), f.score_topk_filtered(I["q"], 10, any_of=I["any"])):
        assert a.tobytes() == b.tobytes()
    for x in (h, f):
        x.close()


def test_refusals_carry_their_messages_write_nothing_and_leave_the_handle_usable():
    import torch
    from sse_amd._lib import SSEError, _ptr
    case = LC.BY_NAME["bias_and_tags"]
    I = LC.inputs(case)
    q = I["q"]
    Q = q.shape[0]
    h = _scorer()
    lse, cnt, bnd = np.full(Q, 123.0), np.full(Q, -7, np.int64), np.full(Q, 123.0)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.array(q)).to(dev)
    md = _i64(I["any"])
    wd = torch.from_numpy(np.array(I["w"])).to(dev)
    d_lse = torch.full((Q,), 123.0, dtype=torch.float64, device=dev)
    d_cnt = torch.full((Q,), -7, dtype=torch.int64, device=dev)
    d_bnd = torch.full((Q,), 123.0, dtype=torch.float64, device=dev)

    def both(scale, masks, weight, message):
        rc = h.lib.sse_score_lse(h._h, _ptr(q), Q, scale, _ptr(I["w"]) if weight else None, _ptr(I["any"]) if masks else None, None,
                                 _ptr(lse), _ptr(cnt), _ptr(bnd))
        assert rc != 0 and h.lib.sse_last_error(h._h).decode() == message, h.lib.sse_last_error(h._h).decode()
        with pytest.raises(SSEError) as ei:
            h.score_lse_dev(qd.data_ptr(), Q, scale, wd.data_ptr() if weight else None, md.data_ptr() if masks else None, None,
                            d_lse.data_ptr(), d_cnt.data_ptr(), d_bnd.data_ptr())
        assert message in str(ei.value)
        torch.cuda.synchronize()
        assert (lse == 123.0).all() and (cnt == -7).all() and (bnd == 123.0).all()
        assert bool((d_lse == 123.0).all()) and bool((d_cnt == -7).all()) and bool((d_bnd == 123.0).all())

    c0 = _counters(h)
    both(64.0, False, False, "sse_score_lse: no index uploaded")
    h.index_upload(I["t"])
    both(0.0, False, False, "sse_score_lse: scale = 0 is not in (0, 256]")
    both(300.0, False, False, "sse_score_lse: scale = 300 is not in (0, 256]")
    both(float("nan"), False, False, "sse_score_lse: scale = nan is not in (0, 256]")
    both(64.0, True, False, "sse_score_lse: tag masks given but the index has no tags (sse_index_set_tags)")
    both(64.0, False, True, "sse_score_lse: q_weight given but the index has no bias (sse_index_set_bias)")
    assert _counters(h) == c0                                 # a refused call is not a call
    h.index_set_tags(I["tags"])                               # after each error the next valid call succeeds
    h.index_set_bias(I["bias"])
    LC.check(case, *h.score_lse(q, case.scale, weight=I["w"], any_of=I["any"], none_of=I["none"]))
    # out_bound may be NULL
    h.score_lse_dev(qd.data_ptr(), Q, case.scale, wd.data_ptr(), md.data_ptr(), None, d_lse.data_ptr(), d_cnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert bool((d_bnd == 123.0).all()) and not bool((d_lse == 123.0).any())
    # Q == 0 succeeds and writes nothing
    l0, n0, b0 = h.score_lse(np.zeros((0, case.S), np.float32), 64.0)
    assert l0.shape == (0,) and n0.shape == (0,) and b0.shape == (0,)
    d_lse.fill_(123.0)
    h.score_lse_dev(qd.data_ptr(), 0, 64.0, None, None, None, d_lse.data_ptr(), d_cnt.data_ptr(), d_bnd.data_ptr())
    torch.cuda.synchronize()
    assert bool((d_lse == 123.0).all())
    h.close()
