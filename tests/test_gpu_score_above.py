"""sse_score_above*: every row of the resident index that scores at least a threshold, per pair (query, threshold), as segments
of per-pair length -- against the ranking the library already certifies (a segment is a prefix of score_topk's row: ids and
score bits), the float64 numpy reference of tests/above_cases.py, the exact-tie / near-tie / shard constructions of
tests/rank_cases.py, a ladder that dials every segment length across the LDS sort's capacity, the capacity contract, the
device-pointer form and the error paths.  Bars: offsets equal, ids equal, scores the same 64 bits."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import above_cases as AC
from tests import rank_cases as RC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

BAND, BRUTE, LONG = "score_above_band_rows", "score_above_bruteforce_pairs", "score_above_long_segments"
I64MAX = np.iinfo(np.int64).max


def _scorer(S=8):
    params = model_params("dual-encoder", 50, 8, 16, 16, S, 4)
    m, _ = make_pair(params)
    return m.handle


@pytest.mark.parametrize("Q,N,S,how", [(65, 4099, 256, "f32"), (65, 4099, 256, "f64"), (65, 4099, 256, "dev"),
                                       (65, 31, 50, "f32"), (9, 1, 50, "f32"),
                                       (40, 700, 300, "f32"), (40, 700, 620, "f32"), (8, 8227, 20, "f32")])
def test_segment_is_a_prefix_of_the_certified_ranking(Q, N, S, how):
    """N = 4099: a partial last tile and 8 index splits; S = 50: not a multiple of 8; N = 1.  Threshold = the score of column
    j of score_topk: the segment is columns 0 .. j, ids and bits.
    The sweep's other instantiations and its other decode (csrc/score_sweep.h): S = 300 (296 < S <= 616) is two pair tiles
    per workgroup, S = 620 one, with 78 k-groups (78 % 4 = 2: the head of the k-loop and its ring); the 200 pairs leave the
    last pair block partial.  N = 8227 = 257 * 32 + 3 is 258 tiles with a partial last one, and choose_nsplit gives 16 splits
    for any number of pairs: doubling goes on while 258 / (2 splits) >= 16, so it stops at 16, and evening out the rounds
    needs 200 tiles per split.  More than 8 splits is the second branch of the workgroup decode and of the grid size;
    S = 20 is 3 k-groups: all head, no ring body."""
    rng = np.random.RandomState(Q + N + S)
    q, t = RC.unit(rng, Q, S), RC.unit(rng, N, S)
    h = _scorer()
    if how == "f32":
        h.index_upload(t)
    elif how == "f64":
        h.index_upload(RC.unit(rng, N, S).astype(np.float64) * (1.0 + 1e-9))     # values that are NOT float32 numbers
    else:
        import torch
        rows = torch.from_numpy(t).to("cuda:0")
        h.index_set_dev(rows.data_ptr(), N, S)
        torch.cuda.synchronize()
    k = min(N, 64)
    sc, ids = h.score_topk(q, k)
    cols = [j for j in (0, 1, 16, 17, 63) if j < k]
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), len(cols))
    thr = sc[:, cols].reshape(-1)
    brute0 = h.get_counter(BRUTE)
    off, gi, gs = h.score_above(q, thr, pair_q)
    want_len = np.tile(np.array(cols) + 1, Q)
    # (random unit vectors: a tie AT column j with column j + 1 would lengthen the segment; rule it out first)
    nxt = [c for c in cols if c + 1 < k]
    assert (sc[:, nxt] > sc[:, [c + 1 for c in nxt]]).all()
    assert np.array_equal(np.diff(off), want_len)
    for p in range(len(thr)):
        qi, n = pair_q[p], want_len[p]
        assert np.array_equal(gi[off[p]:off[p + 1]], ids[qi, :n]), p
        assert np.array_equal(AC.bits(gs[off[p]:off[p + 1]]), AC.bits(sc[qi, :n])), p
    assert h.get_counter(BRUTE) == brute0


def test_float64_oracle_midpoints_and_ieee_thresholds():
    Q, N, S = 33, 571, 64
    rng = np.random.RandomState(7)
    q, t = RC.unit(rng, Q, S), RC.unit(rng, N, S)
    scores = O.scores_f64(q, t.astype(np.float64))
    ssc = -np.sort(-scores, axis=1)
    js = [0, 9, 285, 569]
    mids = np.stack([(ssc[:, j] + ssc[:, j + 1]) / 2 for j in js], 1)                 # [Q, 4]
    half_gap = min(float(np.min(ssc[:, j] - ssc[:, j + 1])) / 2 for j in js)
    print("smallest half-gap between a midpoint and a score: %.3e" % half_gap)
    assert half_gap > 1e-9, half_gap       # no near-tie can decide this case silently (summation orders differ by ~1e-16)
    special = np.stack([np.full(Q, np.inf), np.full(Q, -np.inf), np.full(Q, np.nan), ssc[:, 0] + 1e-3, ssc[:, -1] - 1e-3], 1)
    thr = np.concatenate([mids, special], 1)
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), thr.shape[1])
    h = _scorer()
    h.index_upload(t)
    got = h.score_above(q, thr.reshape(-1), pair_q)
    want = AC.expected_above(scores, pair_q, thr.reshape(-1))
    assert np.array_equal(np.diff(want[0]).reshape(Q, -1), np.broadcast_to([1, 10, 286, 570, 0, N, 0, 0, N], (Q, 9)))
    AC.assert_above_equal(got, want, exact_scores=False)
    assert np.array_equal(h.count_above(q, thr.reshape(-1), pair_q), np.diff(want[0]))


def test_exact_ties_at_the_threshold():
    q, t, copies = RC.exact_ties_case()
    Q, N = q.shape[0], t.shape[0]
    scores = O.scores_f64(q, t.astype(np.float64))
    h = _scorer()
    h.index_upload(t)
    off, ids, sc = h.score_above(q[:1], [scores[0].max()])
    assert ids.tolist() == copies.tolist() and len(copies) == 31          # the 31 maxima of query 0, in id order
    thr = scores[:, 3].copy()                                             # row 3's score, per query: rows 3, N - 1 and every tie
    got = h.score_above(q, thr)
    want = AC.expected_above(scores, np.arange(Q), thr)
    AC.assert_above_equal(got, want)
    for p in range(Q):
        seg = got[1][got[0][p]:got[0][p + 1]]
        tied = np.flatnonzero(scores[p] == thr[p])
        assert 3 in tied and N - 1 in tied
        assert seg[-len(tied):].tolist() == tied.tolist()                 # the ties close the segment, in id order
    up = np.nextafter(thr, np.inf)                                        # all of them excluded
    got_up = h.score_above(q, up)
    AC.assert_above_equal(got_up, AC.expected_above(scores, np.arange(Q), up))
    assert np.array_equal(np.diff(got_up[0]), np.diff(got[0]) - (scores == thr[:, None]).sum(1))


def test_thresholds_below_fp32_resolution():
    q, t, where = RC.near_tie_case(200, 1000)
    scores = O.scores_f64(q, t)
    thr = np.array([0.5 + 100 * 2.0 ** -30, 2 * (0.5 + 100 * 2.0 ** -30)])
    h = _scorer()
    h.index_upload(t)
    band0, brute0 = h.get_counter(BAND), h.get_counter(BRUTE)
    got = h.score_above(q, thr)
    want = AC.expected_above(scores, [0, 1], thr)
    AC.assert_above_equal(got, want)                                      # one product per score: exact
    for p in range(2):
        seg = got[1][got[0][p]:got[0][p + 1]]
        cluster = seg[np.isin(seg, where)]
        assert cluster.tolist() == where[:99:-1].tolist()                 # exactly cluster rows i >= 100, in descending i
    assert h.get_counter(BAND) - band0 >= 200
    assert h.get_counter(BRUTE) == brute0


def test_band_overflow_is_listed_by_the_float64_sweep():
    q, t, where = RC.near_tie_case(5000, 6000)
    scores = O.scores_f64(q, t)
    base = 0.5 + 2500 * 2.0 ** -30
    thr = np.array([base, 2 * base])
    h = _scorer()
    h.index_upload(t)
    brute0 = h.get_counter(BRUTE)
    got = h.score_above(q, thr, cap=2 * t.shape[0])                       # room for any total: ONE call, one counting pass
    want = AC.expected_above(scores, [0, 1], thr)
    for p in range(2):
        seg = want[1][want[0][p]:want[0][p + 1]]
        assert np.isin(seg, where).sum() == 2500
    AC.assert_above_equal(got, want)
    assert h.get_counter(BRUTE) - brute0 == 2                             # 5000 rows in the band of either pair > 4096


def test_every_segment_length_across_the_lds_sort_capacity():
    q, t, pi = AC.ladder_case()
    N = t.shape[0]
    counts = AC.ladder_counts()
    assert {AC.SORT_CAP - 1, AC.SORT_CAP, AC.SORT_CAP + 1, N} <= set(counts.tolist())
    thr = np.array([AC.ladder_threshold(c) for c in counts])
    pair_q = np.zeros(len(thr), np.int32)
    scores = O.scores_f64(q, t.astype(np.float64))
    h = _scorer()
    h.index_upload(t)
    long0, brute0 = h.get_counter(LONG), h.get_counter(BRUTE)
    got = h.score_above(q, thr, pair_q)
    want = AC.expected_above(scores, pair_q, thr)
    assert np.array_equal(np.diff(want[0]), counts)
    AC.assert_above_equal(got, want)
    # 20011 entries do not fit one LDS sort of 16-byte keys: every segment longer than SORT_CAP is merged through global memory
    assert h.get_counter(LONG) - long0 == int((counts > AC.SORT_CAP).sum()) > 0
    assert h.get_counter(BRUTE) == brute0


def test_long_segments_with_a_tie_group_at_every_threshold():
    """quarter_set(61, 3, 20011, 64): every distinct score value of query 0 as a threshold -- a tie group at every one."""
    q, t = RC.quarter_set(61, 3, 20011, 64)
    N = t.shape[0]
    scores = O.scores_f64(q, t.astype(np.float64))
    thr = np.concatenate([np.unique(scores[0]), [-np.inf]])
    pair_q = np.zeros(len(thr), np.int32)
    h = _scorer()
    h.index_upload(t)
    long0 = h.get_counter(LONG)
    got = h.score_above(q, thr, pair_q)
    want = AC.expected_above(scores, pair_q, thr)
    assert len(thr) > 100 and want[0][-1] * 16 > 20e6
    AC.assert_above_equal(got, want)
    assert h.get_counter(LONG) - long0 == int((np.diff(want[0]) > AC.SORT_CAP).sum())
    sc, ids = h.score_topk(q[:1], N)                                      # the -inf pair IS the certified full ranking
    assert np.array_equal(got[1][got[0][-2]:], ids[0]) and np.array_equal(AC.bits(got[2][got[0][-2]:]), AC.bits(sc[0]))


def _raw(h, q, pair_q, thr, cap, lists=True, fill=-7):
    import ctypes as C
    pq, th = np.asarray(pair_q, np.int32), np.asarray(thr, np.float64)
    L = len(pq)
    off = np.full(L + 1, fill, np.int64)
    ids, sc = np.full(max(cap, 1), fill, np.int64), np.full(max(cap, 1), float(fill))
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = h.lib.sse_score_above(h._h, P(q), q.shape[0], P(pq), P(th), L, cap, P(off), P(ids) if lists else None, P(sc) if lists else None)
    return rc, off, ids, sc, h.lib.sse_last_error(h._h).decode()


def test_capacity_contract_and_count_only_form():
    Q, N, S = 17, 1000, 32
    q, t = RC.quarter_set(12, Q, N, S)
    scores = O.scores_f64(q, t.astype(np.float64))
    thr = np.quantile(scores, 0.9, axis=1)
    pair_q = np.arange(Q, dtype=np.int32)
    want = AC.expected_above(scores, pair_q, thr)
    total = int(want[0][-1])
    h = _scorer()
    h.index_upload(t)
    rc, off, ids, sc, _ = _raw(h, q, pair_q, thr, total)                  # cap == total: lists written
    assert rc == 0
    AC.assert_above_equal((off, ids[:total], sc[:total]), want)
    rc, off, ids, sc, _ = _raw(h, q, pair_q, thr, total - 1)              # one short: offsets exact, lists untouched, rc 0
    assert rc == 0 and np.array_equal(off, want[0]) and (ids == -7).all() and (sc == -7.0).all()
    rc, off, ids, sc, _ = _raw(h, q, pair_q, thr, 0, lists=False)         # NULL lists
    assert rc == 0 and np.array_equal(off, want[0])
    o2, i2, s2 = h.score_above(q, thr, pair_q, cap=total - 1)
    assert np.array_equal(o2, want[0]) and i2 is None and s2 is None
    AC.assert_above_equal(h.score_above(q, thr, pair_q, cap=total + 5), want)
    before, _ = h.score_rank(q, pair_q, np.full(Q, I64MAX), pair_score=thr)
    assert np.array_equal(np.diff(off), before)
    assert np.array_equal(h.count_above(q, thr), before)


def test_shards_concatenate_through_id_base():
    q, t = RC.shard_case()
    Q, N = q.shape[0], t.shape[0]
    cut = 2000
    scores = O.scores_f64(q, t.astype(np.float64))
    thr = np.concatenate([scores[:, 10], np.quantile(scores, 0.99, axis=1)])          # row 10's score (== row 4000's), a high cut
    pair_q = np.tile(np.arange(Q, dtype=np.int32), 2)
    h = _scorer()
    h.index_upload(t)
    whole = h.score_above(q, thr, pair_q)
    AC.assert_above_equal(whole, AC.expected_above(scores, pair_q, thr))
    parts = []
    for base, shard in ((0, t[:cut]), (cut, t[cut:])):
        h.index_upload(shard, id_base=base)
        parts.append(h.score_above(q, thr, pair_q))
        AC.assert_above_equal(parts[-1], AC.expected_above(scores[:, base:base + len(shard)], pair_q, thr, id_base=base))
    assert np.array_equal(np.diff(parts[0][0]) + np.diff(parts[1][0]), np.diff(whole[0]))     # counts add
    import torch
    from sse_amd.sharded import merge_above_runs
    L = len(thr)
    pair = torch.cat([torch.repeat_interleave(torch.arange(L), torch.from_numpy(np.diff(p[0]))) for p in parts])
    mo, mi, ms = merge_above_runs(pair, torch.cat([torch.from_numpy(p[2]) for p in parts]), torch.cat([torch.from_numpy(p[1]) for p in parts]), L)
    AC.assert_above_equal((mo.numpy(), mi.numpy(), ms.numpy()), whole)                        # the merged concatenation is the whole
    for p in range(Q):                                                                        # the tie across the cut, in id order
        seg = whole[1][whole[0][p]:whole[0][p + 1]].tolist()
        assert 10 in seg and 4000 in seg and seg.index(10) < seg.index(4000)


def test_more_than_one_chunk_of_pairs():
    Q, N, S, L = 5, 100, 16, 4099
    q, t = RC.quarter_set(13, Q, N, S)
    scores = O.scores_f64(q, t.astype(np.float64))
    rng = np.random.RandomState(14)
    pair_q = rng.randint(0, Q, size=L).astype(np.int32)
    thr = scores[pair_q, rng.randint(0, N, size=L)]                       # every threshold IS a score: ties at each
    h = _scorer()
    h.index_upload(t)
    AC.assert_above_equal(h.score_above(q, thr, pair_q), AC.expected_above(scores, pair_q, thr))


def test_dev_form_on_a_stream_equals_host_form():
    import torch
    Q, N, S, L = 65, 2049, 64, 333
    rng = np.random.RandomState(9)
    q, t = RC.unit(rng, Q, S), RC.unit(rng, N, S)
    pair_q = rng.randint(0, Q, size=L).astype(np.int32)
    h = _scorer()
    h.index_upload(t)
    sc, _ = h.score_topk(q, 64)
    thr = sc[pair_q, rng.randint(0, 64, size=L)]
    want = h.score_above(q, thr, pair_q)
    total = int(want[0][-1])
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        dq, dpq, dthr = torch.from_numpy(q).to(dev), torch.from_numpy(pair_q).to(dev), torch.from_numpy(thr).to(dev)
        outs = []
        for cap in (total + 100, total - 1):
            off = torch.full((L + 1,), -7, dtype=torch.int64, device=dev)
            ids = torch.full((total + 100,), -7, dtype=torch.int64, device=dev)
            scs = torch.full((total + 100,), -7.0, dtype=torch.float64, device=dev)
            h.score_above_dev(dq.data_ptr(), Q, dpq.data_ptr(), dthr.data_ptr(), L, cap, off.data_ptr(), ids.data_ptr(), scs.data_ptr(), st.cuda_stream)
            outs.append((off, ids, scs))
        offc = torch.full((L + 1,), -7, dtype=torch.int64, device=dev)
        h.score_above_dev(dq.data_ptr(), Q, dpq.data_ptr(), dthr.data_ptr(), L, 0, offc.data_ptr(), None, None, st.cuda_stream)
    st.synchronize()
    h.synchronize()
    off, ids, scs = (x.cpu().numpy() for x in outs[0])
    AC.assert_above_equal((off, ids[:total], scs[:total]), want)
    assert (ids[total:] == -7).all() and (scs[total:] == -7.0).all()
    off, ids, scs = (x.cpu().numpy() for x in outs[1])                    # the total does not fit: decided on the device
    assert np.array_equal(off, want[0]) and (ids == -7).all() and (scs == -7.0).all()
    assert np.array_equal(offc.cpu().numpy(), want[0])


def test_errors_leave_outputs_untouched_and_the_handle_usable():
    import sse_amd
    import torch
    Q, N, S = 4, 100, 16
    q, t = RC.quarter_set(15, Q, N, S)
    scores = O.scores_f64(q, t.astype(np.float64))
    h = _scorer()
    rc, off, ids, sc, msg = _raw(h, q, [0, 1], [0.0, 0.0], 50)            # no index set
    assert rc != 0 and "index" in msg and (off == -7).all() and (ids == -7).all() and (sc == -7.0).all()
    h.index_upload(t, id_base=1000)
    for pq in ([0, Q], [-1, 0]):
        rc, off, ids, sc, msg = _raw(h, q, pq, [0.0, 0.0], 500)
        assert rc != 0 and "pair_q" in msg, (rc, msg)
        assert (off == -7).all() and (ids == -7).all() and (sc == -7.0).all()
        with pytest.raises(sse_amd.SSEError):
            h.score_above(q, [0.0, 0.0], pq)
    rc, off, ids, sc, _ = _raw(h, q, [], [], 5)                           # L = 0
    assert rc == 0 and off.tolist() == [0] and (ids == -7).all()
    thr = scores[np.arange(Q), [0, 50, 99, 1]]
    want = AC.expected_above(scores, np.arange(Q), thr, id_base=1000)
    AC.assert_above_equal(h.score_above(q, thr), want)
    # device form: a bad pair surfaces through synchronize(), nothing is written, the next call is served
    dev = torch.device("cuda:0")
    dq, dthr = torch.from_numpy(q).to(dev), torch.from_numpy(thr[:2].copy()).to(dev)
    dpq = torch.tensor([0, Q], dtype=torch.int32, device=dev)
    off = torch.full((3,), -7, dtype=torch.int64, device=dev)
    ids = torch.full((2 * N,), -7, dtype=torch.int64, device=dev)
    sc = torch.full((2 * N,), -7.0, dtype=torch.float64, device=dev)
    h.score_above_dev(dq.data_ptr(), Q, dpq.data_ptr(), dthr.data_ptr(), 2, 2 * N, off.data_ptr(), ids.data_ptr(), sc.data_ptr())
    with pytest.raises(sse_amd.SSEError):
        h.synchronize()
    assert off.cpu().tolist() == [-7, -7, -7] and (ids.cpu().numpy() == -7).all() and (sc.cpu().numpy() == -7.0).all()
    dpq = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    h.score_above_dev(dq.data_ptr(), Q, dpq.data_ptr(), dthr.data_ptr(), 2, 2 * N, off.data_ptr(), ids.data_ptr(), sc.data_ptr())
    h.synchronize()
    n = int(want[0][2])
    AC.assert_above_equal((off.cpu().numpy(), ids.cpu().numpy()[:n], sc.cpu().numpy()[:n]), (want[0][:3], want[1][:n], want[2][:n]))


def test_other_entry_points_see_no_change():
    Q, N, S = 33, 571, 64
    rng = np.random.RandomState(16)
    q, t = RC.unit(rng, Q, S), RC.unit(rng, N, S)
    h = _scorer()
    h.index_upload(t)
    pair_q = np.arange(Q, dtype=np.int32)
    pair_id = rng.randint(0, N, size=Q).astype(np.int64)
    s0, i0 = h.score_topk(q, 20)
    b0, r0 = h.score_rank(q, pair_q, pair_id)
    h.score_above(q, s0[:, 10])
    s1, i1 = h.score_topk(q, 20)
    b1, r1 = h.score_rank(q, pair_q, pair_id)
    assert np.array_equal(i0, i1) and np.array_equal(AC.bits(s0), AC.bits(s1))
    assert np.array_equal(b0, b1) and np.array_equal(AC.bits(r0), AC.bits(r1))


def test_near_duplicate_pairs_and_the_tsv(tmp_path):
    from sse_amd import sse_index
    t = AC.near_duplicate_rows()
    N = t.shape[0]
    scores = O.scores_f64(t, t.astype(np.float64))
    threshold = 0.999
    assert np.abs(scores - threshold).min() > 1e-9                        # no score close enough to flip on summation order
    want = AC.expected_near_duplicates(scores, threshold)
    assert len(want) == 17                                                # 12 planted copies and 5 planted near-copies
    h = _scorer()
    h.index_upload(t)
    got = sse_index.near_duplicate_pairs(h, t, threshold, block=128)      # three blocks of queries
    assert [(i, j) for i, j, _ in got] == [(i, j) for i, j, _ in want]
    assert max(abs(g[2] - w[2]) for g, w in zip(got, want)) < 1e-12
    sc, ids = h.score_topk(t, N)                                          # and the scores are score_topk's bits
    for i, j, s in got:
        assert AC.bits([s])[0] == AC.bits(sc[i, ids[i] == j])[0]
    names = ["tgt%03d" % r for r in range(N)]
    path = os.path.join(str(tmp_path), "nearDuplicates.tsv")
    sse_index.write_near_duplicates(path, names, got)
    back = sse_index.read_near_duplicates(path)
    assert back == [(names[i], names[j], s) for i, j, s in got]           # repr of a float64 round-trips
