"""Top-k above 16 on both of its routes, and two k <= 16 neighbours of the paging code, against the float64 oracle (DESIGN K6;
cases, reference and check in tests/topk_cases.py, proven on the CPU by tests/test_topk_cases_host.py).

Every case runs the host entry (Handle.score_topk) and the device entry (score_topk_dev, every stage queued, outputs
pre-filled with NaN / -7): the two results are np.array_equal, and check() holds them to the oracle -- ids exact, scores
within max(1e-12, two float64 summation orders), no row twice, lower row first in an exact tie.  The counters
score_collect_queries / score_bruteforce_queries are read around each call and must move by what the code says they move
(derivation: tests/topk_cases.py), which is what proves the route.  One TOPKERR line per case (profiles/score_large_k.txt)."""
import numpy as np
import pytest

from tests import topk_cases as TC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu


def _scorer():
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    return m.handle


def _counters(h):
    return h.get_counter("score_collect_queries"), h.get_counter("score_bruteforce_queries")


def _host_topk(h, q, k):
    return h.score_topk(q, k)


def _dev_topk(h, q, k):
    """sse_score_topk_dev: every stage queued (first stage, then lists_rest), no host check in between."""
    import torch
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
    out_s = torch.full((q.shape[0], k), float("nan"), dtype=torch.float64, device=dev)
    out_i = torch.full((q.shape[0], k), -7, dtype=torch.int64, device=dev)
    h.score_topk_dev(qd.data_ptr(), q.shape[0], k, out_s.data_ptr(), out_i.data_ptr())
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def _set_index(h, case, t, keep):
    if case.upload == "dev":
        import torch
        d = torch.from_numpy(np.ascontiguousarray(t, np.float32)).to("cuda:0")
        keep.append(d)
        h.index_set_dev(d.data_ptr(), t.shape[0], t.shape[1], id_base=case.id_base)
        torch.cuda.synchronize()
    else:
        assert t.dtype == (np.float64 if case.upload == "f64" else np.float32)
        h.index_upload(t, id_base=case.id_base)


def _run(case):
    q, t, _ = TC.inputs(case)
    assert TC.preconditions(case)
    h = _scorer()
    keep = []
    _set_index(h, case, t, keep)
    runs = [()]
    for name, values in case.options:
        runs = [r + ((name, v),) for r in runs for v in values]
    first, worst, deltas = None, 0.0, []
    for opts in runs:
        for name, v in opts:
            h.set_option(name, v)
        for entry in (_host_topk, _dev_topk):
            c0, b0 = _counters(h)
            sc, ids = entry(h, q, case.k)
            c1, b1 = _counters(h)
            deltas.append((c1 - c0, b1 - b0))
            if first is None:
                first = (sc, ids)
            else:
                assert np.array_equal(ids, first[1]) and np.array_equal(sc, first[0]), (case, opts, entry.__name__)
            worst = max(worst, TC.check(case, sc, ids))
    tol = TC.scales(case)[2]
    print("TOPKERR %s Q %d N %d S %d k %d base %d %s: worst |score - oracle| %.3e = %.3f tol (bar %.3e), (collect, brute) deltas %s want (%s, %d)"
          % (case.name, case.Q, case.N, case.S, case.k, case.id_base, case.upload, worst, worst / tol, TC.score_bar(case),
             sorted(set(deltas)), "any" if case.collect < 0 else case.collect, case.brute))
    for dc, db in deltas:
        assert db == case.brute, (case, deltas)
        assert case.collect < 0 or dc == case.collect, (case, deltas)
    return first


@pytest.mark.parametrize("case", [c for c in TC.CASES if not c.name.startswith("strided_open")], ids=repr)
def test_large_k_case(case):
    sc, ids = _run(case)
    if case.name == "second_pool":                            # the last 32 rows as strictly as the first: on their own
        ws, wi = TC.expected(case)
        assert np.array_equal(ids[-32:], wi[-32:]) and np.abs(sc[-32:] - ws[-32:]).max() <= TC.score_bar(case)


def test_f64_rows_and_their_rounding_differ_on_the_device_as_in_the_oracle():
    """Each is checked against its own reference above; here: the float64 index really reaches the float64 dot (a scorer
    that re-scored the float32 image would return the rounded rows' scores for both)."""
    a, b = TC.BY_NAME["f64_rows"], TC.BY_NAME["f64_rows_rounded"]
    out = []
    for c in (a, b):
        h = _scorer()
        h.index_upload(TC.inputs(c)[1], id_base=c.id_base)
        out.append(h.score_topk(TC.inputs(c)[0], c.k)[0])
    want = TC.expected(a)[0] - TC.expected(b)[0]
    assert np.abs(want).max() > 1e3 * TC.score_bar(a)
    assert np.abs((out[0] - out[1]) - want).max() <= 2 * TC.score_bar(a)


def test_strided_brute_force_with_open_queries():
    """k = 10.  The follow-up launches of a k <= 16 call are bounded to 2 * cu_count workgroups; with more queries than that
    the strided kernel walks them, and four of them -- first and last of the batch, two in between -- are open.  On the 256
    CUs of an MI355X the grid is 512 and Q = 600; a larger device gets a larger Q."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = TC.BY_NAME["strided_open_q600"] if cus <= 300 else TC.strided_case(2 * cus + 88)
    assert case.Q > 2 * cus
    _run(case)
