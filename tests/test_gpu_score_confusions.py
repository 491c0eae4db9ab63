"""sse_score_confusions against the float64 oracle (DESIGN K6k; cases, reference and check in tests/confusion_cases.py, proven on
the CPU by tests/test_confusion_cases_host.py).

Every case runs the host entry (Handle.score_confusions), the device entry on the null stream (score_confusions_dev, outputs
pre-filled with NaN / -7) and the device entry queued twice on a side stream with no wait between the calls: the results are
np.array_equal and check() holds them to the oracle -- ids, counts and best positive ids exact, padding exact, no positive, no
row below the floor, lower row first in an exact tie, scores within max(1e-12, two float64 summation orders).  The three
score_confusions_* counters are read around each call.  On the same handle, bit for bit: the columns are those of
score_topk_filtered(exclude = positives) cut at pos_scores - margin in numpy float64, and pos_scores is score_rank's out_score
of (q, pos_ids[q]).  One CONFR line per case."""
import numpy as np
import pytest

from tests import confusion_cases as CC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

NAMES = ("score_confusions_collected_rows", "score_confusions_bruteforce_queries", "score_confusions_floor_queries")


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _counters(h):
    return tuple(h.get_counter(n) for n in NAMES)


def _host(h, q, k, pos, margin):
    return h.score_confusions(q, k, pos, margin)


def _dev_calls(h, q, k, pos, margin, stream, times):
    import torch
    dev = torch.device("cuda:0")
    Q = q.shape[0]
    outs = []
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.default_stream()):
        qd = torch.from_numpy(np.array(q, dtype=np.float32)).to(dev)
        pd = torch.from_numpy(np.array(pos, dtype=np.int64)).to(dev)
        for _ in range(times):
            o = (torch.full((Q, k), float("nan"), dtype=torch.float64, device=dev), torch.full((Q, k), -7, dtype=torch.int64, device=dev),
                 torch.full((Q,), -7, dtype=torch.int32, device=dev), torch.full((Q,), float("nan"), dtype=torch.float64, device=dev),
                 torch.full((Q,), -7, dtype=torch.int64, device=dev))
            h.score_confusions_dev(qd.data_ptr(), Q, k, pd.data_ptr(), pos.shape[1], margin, o[0].data_ptr(), o[1].data_ptr(),
                                   o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            outs.append(o)
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy() for t in o) for o in outs]


def _dev(h, q, k, pos, margin):
    return _dev_calls(h, q, k, pos, margin, None, 1)[0]


def _queued(h, q, k, pos, margin):
    import torch
    a, b = _dev_calls(h, q, k, pos, margin, torch.cuda.Stream(), 2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    return b


def _set_index(h, case, keep):
    t = CC.inputs(case)["t"]
    if case.upload == "dev":
        import torch
        d = torch.from_numpy(np.array(t, dtype=np.float32)).to("cuda:0")
        keep.append(d)
        h.index_set_dev(d.data_ptr(), t.shape[0], t.shape[1], id_base=case.id_base)
        torch.cuda.synchronize()
    else:
        assert t.dtype == (np.float64 if case.upload == "f64" else np.float32)
        h.index_upload(t, id_base=case.id_base)


def _cut_on_host(fs, fi, fc, floor, k):
    """the filtered call's columns with the rows below `floor` removed (a prefix: the list is sorted), padded"""
    ws = np.full((fs.shape[0], k), -np.inf)
    wi = np.full((fs.shape[0], k), CC.PAD_ID, np.int64)
    wc = np.zeros(fs.shape[0], np.int32)
    for qi in range(fs.shape[0]):
        c = int((fs[qi, :fc[qi]] >= floor[qi]).sum())
        ws[qi, :c], wi[qi, :c], wc[qi] = fs[qi, :c], fi[qi, :c], c
    return ws, wi, wc


@pytest.mark.parametrize("case", CC.CASES, ids=repr)
def test_confusion_case(case):
    I = CC.inputs(case)
    assert CC.preconditions(case)
    h = _scorer()
    keep = []
    _set_index(h, case, keep)
    q, pos = I["q"], I["pos"]
    first, worst, log = None, 0.0, []
    for entry, calls in ((_host, 1), (_dev, 1), (_queued, 2)):
        c0 = _counters(h)
        res = entry(h, q, case.k, pos, case.margin)
        d = tuple((b - a) // calls for a, b in zip(c0, _counters(h)))
        log.append((entry.__name__, d))
        if first is None:
            first = res
        else:
            assert all(np.array_equal(x, y) for x, y in zip(res, first)), (case, entry.__name__)
        worst = max(worst, CC.check(case, *res))
        assert d[1] == case.brute, (case, log)
        assert d[0] >= CC.collected_min(case), (case, log, CC.collected_min(case))
        assert d[2] >= 0 and (case.floor is None or d[2] == case.floor), (case, log)
    print("CONFR %s Q %d N %d S %d k %d n_pos %d margin %g base %d %s: worst |score - oracle| %.3e (bar %.3e), counts %s, "
          "(entry, (collected, brute, floor)) %s" % (case.name, case.Q, case.N, case.S, case.k, pos.shape[1], case.margin, case.id_base,
                                                     case.upload, worst, CC.score_bar(case), first[2].tolist(), log))
    sc, ids, cnt, pm, pb = first
    # the filtered call of the same handle, cut on the host at the device's own floor
    fs, fi, fc = h.score_topk_filtered(q, case.k, exclude=pos)
    with np.errstate(invalid="ignore"):
        floor = pm - np.float64(case.margin)
    ws, wi, wc = _cut_on_host(fs, fi, fc, floor, case.k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws) and np.array_equal(cnt, wc), case
    # the best positive's score is the rank call's, bit for bit
    have = np.flatnonzero(pb != CC.PAD_ID)
    if have.size:
        _, rs = h.score_rank(q, have.astype(np.int32), pb[have])
        assert np.array_equal(rs, pm[have]), case
    h.close()


def test_argument_errors_write_nothing_and_leave_the_handle_usable():
    import torch
    from sse_amd._lib import SSEError, _ptr
    case = CC.BY_NAME["three_above_margin0"]
    I = CC.inputs(case)
    q, pos = I["q"], I["pos"]
    Q = q.shape[0]
    wide = np.full((Q, 65), -1, np.int64)
    h = _scorer()
    sc = np.full((Q, 1025), 123.0)
    ids = np.full((Q, 1025), -7, np.int64)
    cnt = np.full(Q, -7, np.int32)
    pm = np.full(Q, 123.0)
    pb = np.full(Q, -7, np.int64)
    dev = torch.device("cuda:0")
    qd, wd = torch.from_numpy(np.array(q)).to(dev), torch.from_numpy(wide).to(dev)
    d_sc = torch.full((Q, 1025), 123.0, dtype=torch.float64, device=dev)
    d_ids = torch.full((Q, 1025), -7, dtype=torch.int64, device=dev)
    d_cnt = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    d_pm = torch.full((Q,), 123.0, dtype=torch.float64, device=dev)
    d_pb = torch.full((Q,), -7, dtype=torch.int64, device=dev)

    def both(match, k=10, n_pos=3, margin=0.0, null_pos=False):
        rc = h.lib.sse_score_confusions(h._h, _ptr(q), Q, k, None if null_pos else _ptr(wide), n_pos, margin, _ptr(sc), _ptr(ids),
                                        _ptr(cnt), _ptr(pm), _ptr(pb))
        assert rc != 0 and match in h.lib.sse_last_error(h._h).decode(), h.lib.sse_last_error(h._h)
        with pytest.raises(SSEError, match=match):
            h.score_confusions_dev(qd.data_ptr(), Q, k, None if null_pos else wd.data_ptr(), n_pos, margin, d_sc.data_ptr(),
                                   d_ids.data_ptr(), d_cnt.data_ptr(), d_pm.data_ptr(), d_pb.data_ptr())
        torch.cuda.synchronize()
        assert (sc == 123.0).all() and (ids == -7).all() and (cnt == -7).all() and (pm == 123.0).all() and (pb == -7).all()
        for t, v in ((d_sc, 123.0), (d_ids, -7), (d_cnt, -7), (d_pm, 123.0), (d_pb, -7)):
            assert bool((t == v).all())

    def valid():
        CC.check(case, *h.score_confusions(q, case.k, pos, case.margin))

    both("no index")
    h.index_upload(I["t"])
    for kw, match in ((dict(k=0), "k = 0"), (dict(k=1025), "k = 1025"), (dict(n_pos=0), "n_pos = 0"), (dict(n_pos=65), "n_pos = 65"),
                      (dict(margin=float("nan")), "margin = nan"), (dict(margin=-np.inf), "margin = -inf"),
                      (dict(null_pos=True), "pos_ids is NULL")):
        both(match, **kw)
        valid()                                               # after each error the next valid call succeeds
    # Q == 0 succeeds and writes nothing; the best-positive outputs may be left out
    r0 = h.score_confusions(np.zeros((0, case.S), np.float32), 10, np.zeros((0, 1), np.int64))
    assert r0[0].shape == (0, 10) and r0[2].shape == (0,) and r0[3].shape == (0,)
    h.score_confusions_dev(qd.data_ptr(), 0, 10, wd.data_ptr(), 3, 0.0, d_sc.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert bool((d_sc == 123.0).all()) and bool((d_cnt == -7).all())
    pd = torch.from_numpy(np.array(pos)).to(dev)
    o_s = torch.empty((Q, case.k), dtype=torch.float64, device=dev)
    o_i = torch.empty((Q, case.k), dtype=torch.int64, device=dev)
    o_c = torch.empty((Q,), dtype=torch.int32, device=dev)
    h.score_confusions_dev(qd.data_ptr(), Q, case.k, pd.data_ptr(), pos.shape[1], case.margin, o_s.data_ptr(), o_i.data_ptr(), o_c.data_ptr())
    torch.cuda.synchronize()
    ws, wi, wc, wm, wb = CC.expected(case)
    CC.check(case, o_s.cpu().numpy(), o_i.cpu().numpy(), o_c.cpu().numpy(), wm, wb)
    # a list of lists is padded with -1, as sse_index.hard_negatives pads
    ragged = [[int(v) for v in row if v >= 0][:1 + qi % 2] for qi, row in enumerate(pos)]
    CC.check(case, *h.score_confusions(q, case.k, ragged, case.margin))
    h.close()
