"""Parity of the HIP LSTM encoder (through the C ABI) against the CPU oracle.
Tolerance: |delta| <= 1e-4 per component on l2-normalised encodings (the
north-star budget is 1e-3 on cosines); fp32 MFMA vs fp32 BLAS ordering only."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import make_pair, model_params, random_ids

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _ran(h, before, **moved):
    """The LSTM path counters named (include/sse_hip.h) moved by the given amounts since `before` = _paths(h)."""
    now = _paths(h)
    got = {n: now[n] - before[n] for n in moved}
    assert got == moved, (got, moved)


def _paths(h):
    return {n: h.get_counter(n) for n in ("lstm_path_persist", "lstm_path_cluster", "lstm_path_small", "lstm_path_fwd",
                                          "lstm_fwd_rows32", "lstm_fwd_rows64", "lstm_fwd_gate_split", "lstm_fwd_x_table")}

CASES = [
    # mode, V, E, Hs, Ht, S, T, B
    ("dual-encoder", 500, 50, 256, 256, 256, 32, 70),      # BASELINE configs[1] shape
    ("shared-encoder", 300, 40, 96, 96, 50, 50, 33),       # makefile:42 crosslingual recipe
    ("shared-encoder", 300, 50, 128, 128, 64, 80, 65),     # BASELINE configs[0] shape
    ("dual-encoder", 120, 30, 128, 64, 64, 7, 1),          # ranking recipe sizes, B = 1 (demo)
    ("dual-encoder", 64, 50, 96, 200, 64, 2, 129),         # T = 2 minimum, odd cell sizes
    ("source-encoder-only", 64, 8, 32, 32, 16, 5, 3),
    ("dual-encoder", 200, 50, 512, 300, 128, 12, 45),      # cell sizes up to 512 (32-row tiles, 2 unit blocks per wave)
    ("dual-encoder", 500, 50, 256, 256, 256, 32, 9000),    # > 8192 rows: 64-row tiles; below: 32-row tiles
    ("dual-encoder", 300, 50, 96, 80, 64, 12, 9000),       # reference default cell size at 64-row tiles: three live unit blocks, block 2 split by pass
    ("shared-encoder", 300, 40, 72, 72, 50, 9, 8300),      # three live unit blocks with a partial last one
    ("dual-encoder", 200, 40, 64, 40, 50, 10, 8500),        # H <= 64 at 64-row tiles: two live unit blocks
]


@pytest.mark.parametrize("small_rows", [1024, 0])         # few-sequences kernel for B <= 1024 (default) / matrix kernel only
@pytest.mark.parametrize("mode,V,E,Hs,Ht,S,T,B", CASES)
def test_encode_matches_oracle(mode, V, E, Hs, Ht, S, T, B, small_rows):
    params = model_params(mode, V, E, Hs, Ht, S, T)
    m, p = make_pair(params, seed=1)
    m.handle.set_option("lstm_small_rows", small_rows)
    if small_rows == 0:
        m.handle.set_option("lstm_persist_rows", 0)       # matrix kernel only
    rng = np.random.RandomState(3)
    ids = random_ids(rng, B, T, V, pad_frac=0.7)
    sides = ("src", "tgt") if mode != "source-encoder-only" else ("src",)
    for side in sides:
        for normalize in (True, False):
            want = O.encode(p, params, side, ids, normalize=normalize)
            got = (m.encode_source if side == "src" else m.encode_target)(ids, normalize=normalize)
            assert got.shape == want.shape and got.dtype == np.float32
            scale = 1.0 if normalize else max(1.0, float(np.abs(want).max()))
            assert np.abs(got - want).max() <= TOL * scale, (side, normalize, np.abs(got - want).max())
            if normalize:
                cos = np.sum(got.astype(np.float64) * want, axis=1)
                assert cos.min() > 1 - 1e-6


def test_all_pad_rows_and_duplicates():
    params = model_params("dual-encoder", 100, 50, 96, 96, 64, 20)
    m, p = make_pair(params, seed=2)
    ids = np.zeros((5, 20), np.int32)
    ids[:, -1] = 1
    ids[3, 5:10] = 7
    got = m.encode_source(ids)
    want = O.encode(p, params, "src", ids)
    assert np.abs(got - want).max() <= TOL
    assert np.array_equal(got[0], got[1])           # identical rows -> identical encodings


def test_long_sequence_T1000():
    """rawdata-qna recipe: max_seq_length=1000 (makefile:17)."""
    params = model_params("dual-encoder", 200, 50, 96, 96, 64, 1000)
    m, p = make_pair(params, seed=4)
    ids = random_ids(np.random.RandomState(0), 3, 1000, 200, pad_frac=0.9)
    got = m.encode_target(ids)
    want = O.encode(p, params, "tgt", ids)
    assert np.abs(got - want).max() <= TOL


def test_out_of_range_id_raises():
    import sse_amd
    params = model_params("dual-encoder", 50, 8, 16, 16, 8, 4)
    m, _ = make_pair(params)
    ids = np.array([[0, 3, 50, 1]], np.int32)
    with pytest.raises(sse_amd.SSEError):
        m.encode_source(ids)
    ok = m.encode_source(np.array([[0, 3, 49, 1]], np.int32))   # handle stays usable
    assert np.isfinite(ok).all()


def test_session_run_contract():
    """sess.run([model.norm_tgt_seq_embedding], feed) returns a one-element list
    that callers np.vstack (sse_index.py:90-92)."""
    import sse_amd
    params = model_params("shared-encoder", 80, 16, 32, 32, 24, 6)
    m, p = make_pair(params)
    sess = sse_amd.Session(m)
    ids = random_ids(np.random.RandomState(1), 4, 6, 80).tolist()
    out = sess.run([m.norm_tgt_seq_embedding], feed_dict=m.get_target_encoding_feed_dict(ids))
    assert isinstance(out, list) and len(out) == 1
    enc = np.vstack(out)
    assert np.abs(enc - O.encode(p, params, "tgt", np.array(ids))).max() <= TOL
    raw = np.vstack(sess.run([m.src_seq_embedding], feed_dict=m.get_source_encoding_feed_dict(ids)))
    assert np.abs(raw - O.encode(p, params, "src", np.array(ids), normalize=False)).max() <= TOL * max(1, np.abs(raw).max())


def test_large_batch_property_rows_independent():
    """BASELINE-size batch: every row equals the same sequence encoded alone
    in a small batch (size-independent property; oracle only on a sample)."""
    params = model_params("dual-encoder", 32000, 50, 256, 256, 256, 32)
    m, p = make_pair(params, seed=5)
    rng = np.random.RandomState(9)
    ids = random_ids(rng, 16384 + 37, 32, 32000)
    big = m.encode_source(ids)
    assert np.allclose(np.linalg.norm(big, axis=1), 1.0, atol=1e-5)
    pick = rng.choice(len(ids), 96, replace=False)
    m.handle.set_option("lstm_small_rows", 0)        # matrix kernel for the small batch too
    m.handle.set_option("lstm_persist_rows", 0)
    small = m.encode_source(ids[pick])
    assert np.array_equal(small, big[pick])          # bit-identical: no cross-row coupling
    # the few-sequences kernel (same fma chains in the same order on the vector ALUs) agrees to the last bits
    m.handle.set_option("lstm_small_rows", 1024)
    few = m.encode_source(ids[pick])
    print("few-sequences kernel vs matrix kernel: max |d| = %.3g, bit-identical rows: %d / %d"
          % (np.abs(few - small).max(), int(np.all(few == small, axis=1).sum()), len(pick)))
    assert np.array_equal(few, small)
    one = np.concatenate([m.encode_source(ids[pick[i:i + 1]]) for i in range(8)])
    assert np.array_equal(one, few[:8])              # and is itself independent of the batch it runs in
    # the weights-in-LDS cluster kernel (<= 32 rows): the same bits again, alone and in a batch
    m.handle.set_option("lstm_persist_rows", 32)
    one = np.concatenate([m.encode_source(ids[pick[i:i + 1]]) for i in range(4)])
    assert np.array_equal(one, few[:4])
    assert np.array_equal(m.encode_source(ids[pick[:29]]), few[:29])
    want = O.encode(p, params, "src", ids[pick[:16]])
    assert np.abs(small[:16] - want).max() <= TOL


@pytest.mark.parametrize("mode,V,E,Hs,Ht,S,T", [
    ("dual-encoder", 500, 50, 256, 256, 256, 32),          # configs[1]: 16 workgroups x 16 units
    ("shared-encoder", 300, 50, 96, 96, 64, 80),           # reference defaults: 6 units per workgroup
    ("dual-encoder", 200, 50, 512, 300, 128, 12),          # 32 workgroups per cluster; 300 = 19 units each, uneven tail
    ("dual-encoder", 90, 8, 16, 40, 512, 9),               # tiny cells, widest encoding
])
def test_cluster_kernel_equals_the_other_kernels(mode, V, E, Hs, Ht, S, T):
    """lstm_persist.hip (weights resident in LDS, h_t exchanged between the workgroups of a cluster every step) for
    1 .. 32 rows: bit-identical to the few-sequences kernel (which the matrix kernel equals), with and without the
    pad-prefix skip, within the encoder tolerance of the oracle."""
    params = model_params(mode, V, E, Hs, Ht, S, T)
    m, p = make_pair(params, seed=8)
    rng = np.random.RandomState(2)
    for B in (1, 3, 4, 5, 17, 32):
        ids = random_ids(rng, B, T, V, pad_frac=0.6)
        if B == 5:
            ids[2, :] = 0
            ids[2, -1] = 1                                 # only EOS
            ids[4] = rng.randint(2, V, size=T)             # no padding at all
        for side, enc in (("src", m.encode_source), ("tgt", m.encode_target)):
            for normalize in (True, False):
                m.handle.set_option("lstm_persist_rows", 0)
                n0 = _paths(m.handle)
                ref = enc(ids, normalize=normalize)
                _ran(m.handle, n0, lstm_path_small=1, lstm_path_persist=0)
                m.handle.set_option("lstm_persist_rows", 32)
                n0 = _paths(m.handle)
                got = enc(ids, normalize=normalize)
                # cells above 256 units need 32 workgroups per cluster, 8 x 32 x 2 = 512 compute units for the chooser's
                # co-residency rule: on a 256-CU device they stay on the few-sequences kernel
                if (Hs if side == "src" else Ht) <= 256:
                    _ran(m.handle, n0, lstm_path_persist=1, lstm_path_small=0)
                else:
                    _ran(m.handle, n0, lstm_path_persist=0, lstm_path_small=1)
                assert np.array_equal(got, ref), (B, side, normalize, np.abs(got - ref).max())
                m.handle.set_option("pad_skip", 0)
                assert np.array_equal(enc(ids, normalize=normalize), ref)
                m.handle.set_option("pad_skip", 1)
        want = O.encode(p, params, "src", ids)
        assert np.abs(m.encode_source(ids) - want).max() <= TOL
    import sse_amd
    bad = random_ids(rng, 2, T, V)
    bad[1, -1] = V
    with pytest.raises(sse_amd.SSEError):
        m.encode_source(bad)
    assert np.isfinite(m.encode_source(random_ids(rng, 2, T, V))).all()


def test_cluster_kernel_survives_many_calls_and_shape_changes():
    """The cluster kernel's exchange buffers are reused across calls with a per-call tag epoch: thousands of calls that
    alternate sides (different cell sizes -> different exchange layouts), batch sizes and sequence lengths must keep
    returning exactly the few-sequences kernel's result (a stale tag would read another call's h_t)."""
    params = model_params("dual-encoder", 400, 50, 256, 96, 64, 24)
    m, p = make_pair(params, seed=21)
    rng = np.random.RandomState(6)
    cases = []
    for B, T in ((1, 24), (5, 7), (32, 24), (2, 2), (17, 13)):
        ids = random_ids(rng, B, T, 400, pad_frac=0.4)
        m.handle.set_option("lstm_persist_rows", 0)
        ref = (m.encode_source(ids), m.encode_target(ids))
        cases.append((ids, ref))
    m.handle.set_option("lstm_persist_rows", 32)
    for it in range(1500):
        ids, ref = cases[it % len(cases)]
        side = it % 2
        got = (m.encode_source if side == 0 else m.encode_target)(ids)
        if it % 97 == 0 or it > 1480:
            assert np.array_equal(got, ref[side]), it
    assert np.array_equal(m.encode_source(cases[0][0]), cases[0][1][0])
    # the 20-bit epoch runs out: the buffers are cleared and the epochs restart -- no stale tag can match
    m.handle.set_option("lstm_persist_epoch", (1 << 20) - 4)
    for it in range(10):
        ids, ref = cases[it % len(cases)]
        assert np.array_equal(m.encode_source(ids), ref[0]), it


@pytest.mark.parametrize("mode,V,E,Hs,Ht,S,T,B,pad", [
    ("dual-encoder", 500, 50, 256, 256, 256, 32, 1200, 0.0),      # configs[1] shape
    ("dual-encoder", 300, 50, 200, 160, 64, 80, 1100, 0.7),       # padded cells / units, long left-padded rows
    ("shared-encoder", 120, 8, 256, 256, 100, 2, 1030, 0.3),      # T = 2, narrow embedding (one x group)
    ("shared-encoder", 300, 50, 96, 96, 64, 80, 1100, 0.6),       # reference defaults: Hp = 128 mapping, 3 live unit blocks
    ("dual-encoder", 300, 30, 128, 40, 50, 13, 1500, 0.2),        # Hp = 128 full / mostly padding cells
])
def test_split_bf16_matrix_path_stays_within_the_encoder_tolerance(mode, V, E, Hs, Ht, S, T, B, pad):
    """Option lstm_x3 (lstm_fwd_x3.hip): gate GEMMs as three bf16 MFMAs on hi + lo split operands.  Not the fp32
    arithmetic -- the claim is the tolerance: within 1e-4 of the oracle per component (north-star budget 1e-3; observed
    ~1e-5) and within 5e-5 of the exact fp32 kernel, over T = 2 .. 80 recurrent steps."""
    params = model_params(mode, V, E, Hs, Ht, S, T)
    m, p = make_pair(params, seed=13)
    rng = np.random.RandomState(4)
    ids = random_ids(rng, B, T, V, pad_frac=pad)
    for side, enc in (("src", m.encode_source), ("tgt", m.encode_target)):
        for normalize in (True, False):
            m.handle.set_option("lstm_x3", 0)
            exact = enc(ids, normalize=normalize)
            m.handle.set_option("lstm_x3", 1)
            got = enc(ids, normalize=normalize)
            want = O.encode(p, params, side, ids[:200], normalize=normalize)
            scale = 1.0 if normalize else max(1.0, float(np.abs(want).max()))
            d_exact, d_oracle = np.abs(got - exact).max() / scale, np.abs(got[:200] - want).max() / scale
            m.handle.set_option("pad_skip", 0)
            assert np.array_equal(enc(ids, normalize=normalize), got)     # the left-pad prefix skip is exact on this path too
            m.handle.set_option("pad_skip", 1)
            print("lstm_x3 %s normalize=%d: |x3 - fp32 kernel| %.2e, |x3 - oracle| %.2e" % (side, normalize, d_exact, d_oracle))
            if (Hs if side == "src" else Ht) >= 64:
                assert 0 < d_exact < 5e-5 and d_oracle < TOL
            else:                      # cells below 64 units keep the exact fp32 kernel
                assert d_exact == 0 and d_oracle < TOL
            if normalize:
                assert np.sum(got.astype(np.float64) * exact, axis=1).min() > 1 - 1e-6    # fp32 norms: 1 +- 2e-7
    # the split copies follow a weight update
    m.handle.set_option("lstm_x3", 0)


def test_pad_prefix_skip_is_bit_identical_and_survives_weight_updates():
    """Option pad_skip: tiles start after their common left-PAD prefix from a precomputed state
    (same kernel arithmetic) -- results must equal the full T-step run bit for bit."""
    params = model_params("dual-encoder", 300, 50, 256, 96, 64, 40)
    m, p = make_pair(params, seed=6)
    rng = np.random.RandomState(12)
    ids = random_ids(rng, 300, 40, 300, pad_frac=0.95)
    ids[7, :] = 0
    ids[7, -1] = 1                                        # only EOS
    ids[8, :] = rng.randint(2, 300, size=40)              # no padding at all
    ids[8, -1] = 1
    for side, enc in (("src", m.encode_source), ("tgt", m.encode_target)):
        m.handle.set_option("pad_skip", 1)
        fast = enc(ids)
        m.handle.set_option("pad_skip", 0)
        full = enc(ids)
        assert np.array_equal(fast, full), side
        assert np.abs(full - O.encode(p, params, side, ids)).max() <= TOL
    # a weight change invalidates the prefix table
    m.handle.set_option("pad_skip", 1)
    p2 = {k: (v * 1.1).astype(np.float32) for k, v in p.items()}
    m.set_variables(p2)
    assert np.abs(m.encode_source(ids) - O.encode(p2, params, "src", ids)).max() <= TOL
    # a small (unsorted, single-tile) batch with a PAD in the middle of a sequence
    ids2 = ids[:5].copy()
    ids2[2, 20] = 0
    assert np.abs(m.encode_source(ids2) - O.encode(p2, params, "src", ids2)).max() <= TOL


def test_in_graph_predict_and_similarity():
    """`_def_predict` / `self.similarity` (sse_model.py:286,344-352): never fetched by the reference's
    CLIs but part of the model surface."""
    import sse_amd
    params = model_params("dual-encoder", 90, 16, 32, 32, 24, 7)
    m, p = make_pair(params, seed=9)
    rng = np.random.RandomState(2)
    src, tgt = random_ids(rng, 6, 7, 90), random_ids(rng, 21, 7, 90)
    ns, nt = O.encode(p, params, "src", src), O.encode(p, params, "tgt", tgt)
    sim = O.similarity(ns, nt)
    sess = sse_amd.Session(m)
    scores, labels = sess.run([m.predicted_tgts_score, m.predicted_labels], feed_dict=m.get_predict_feed_dict(src, tgt))
    want_idx = np.argsort(-sim, axis=1, kind="stable")[:, :10]
    want_sc = np.take_along_axis(sim, want_idx, axis=1)
    want_sc = want_sc / np.linalg.norm(want_sc, axis=1, keepdims=True)
    assert np.array_equal(labels, want_idx)
    assert np.abs(scores - want_sc).max() < 1e-5
    got_sim = sess.run(m.similarity, feed_dict=m.get_predict_feed_dict(src, tgt))
    assert np.abs(got_sim - sim).max() < 1e-5


def test_in_graph_predict_and_similarity_at_encoding_size_512():
    """The same two fetches at configs[4]'s encoding size (S = 512: the scorer's 64-query LDS blocks), with more
    than 64 source rows and a target batch larger than one index tile (sse_model.py:286,344-352)."""
    import sse_amd
    params = model_params("dual-encoder", 120, 16, 64, 64, 512, 9)
    m, p = make_pair(params, seed=10)
    rng = np.random.RandomState(3)
    src, tgt = random_ids(rng, 70, 9, 120), random_ids(rng, 45, 9, 120)
    ns, nt = O.encode(p, params, "src", src), O.encode(p, params, "tgt", tgt)
    gs, gt = m.encode_source(src), m.encode_target(tgt)
    assert np.abs(gs - ns).max() < 1e-4 and np.abs(gt - nt).max() < 1e-4
    sess = sse_amd.Session(m)
    scores, labels = sess.run([m.predicted_tgts_score, m.predicted_labels], feed_dict=m.get_predict_feed_dict(src, tgt))
    # ranking parity on identical inputs (the GPU's own encodings), values against the oracle's encodings
    assert np.array_equal(labels, O.topk(O.scores_f64(gs, gt.astype(np.float64)), 10)[1])
    sim = O.similarity(ns, nt)
    want_sc = np.take_along_axis(sim, labels, axis=1)
    want_sc = want_sc / np.linalg.norm(want_sc, axis=1, keepdims=True)
    assert np.abs(scores - want_sc).max() < 1e-4
    got_sim = sess.run(m.similarity, feed_dict=m.get_predict_feed_dict(src, tgt))
    assert got_sim.shape == (70, 45) and np.abs(got_sim - sim).max() < 1e-4


def test_concurrent_encode_and_score_from_threads():
    """webserver.py:108 calls sess.run from Flask worker threads on ONE session; the handle serialises
    encode / score calls internally (include/sse_hip.h): results equal the single-threaded ones."""
    import threading
    params = model_params("dual-encoder", 300, 50, 96, 96, 64, 20)
    m, _ = make_pair(params, seed=12)
    rng = np.random.RandomState(5)
    tgt = random_ids(rng, 400, 20, 300, 0.5)
    m.handle.index_upload(m.encode_target(tgt).astype(np.float64))
    batches = [random_ids(rng, b, 20, 300, 0.5) for b in (1, 7, 64, 130, 600, 33, 2, 257)]
    want = []
    for ids in batches:
        enc = m.encode_source(ids)
        want.append((enc, m.handle.score_topk(enc, 10)))
    got, errs = [None] * len(batches), []

    def work(i):
        try:
            for _ in range(5):
                enc = m.encode_source(batches[i])
                got[i] = (enc, m.handle.score_topk(enc, 10))
        except Exception as ex:                                 # pragma: no cover
            errs.append(ex)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(batches))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs
    for (we, (ws, wi)), (ge, (gs, gi)) in zip(want, got):
        assert np.array_equal(we, ge) and np.array_equal(wi, gi) and np.array_equal(ws, gs)


def test_cluster_kernel_miss_falls_back_to_the_few_sequences_kernel():
    """A cluster workgroup that does not arrive (device busy) used to fail the request; the host-buffer entry points now
    re-run the batch on lstm_small -- bit-identical results -- and count it (option lstm_persist_inject_miss simulates
    the condition after every cluster launch)."""
    params = model_params("dual-encoder", 300, 50, 96, 96, 64, 20)
    m, _ = make_pair(params, seed=13)
    rng = np.random.RandomState(6)
    ids = random_ids(rng, 5, 20, 300, 0.5)
    tgt = random_ids(rng, 200, 20, 300, 0.5)
    m.handle.index_upload(m.encode_target(tgt).astype(np.float64))
    want = m.encode_source(ids)
    want_s, want_i = m.handle.encode_score_topk(0, ids, False, 7)
    assert m.handle.get_counter("lstm_persist_fallbacks") == 0
    m.handle.set_option("lstm_cluster_backoff", 0)              # (every call tries the cluster kernel again: counted below)
    m.handle.set_option("lstm_persist_inject_miss", 1)
    got = m.encode_source(ids)
    got_s, got_i = m.handle.encode_score_topk(0, ids, False, 7)
    m.handle.set_option("lstm_persist_inject_miss", 0)
    assert np.array_equal(got, want) and np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)
    assert m.handle.get_counter("lstm_persist_fallbacks") == 2
    assert np.array_equal(m.encode_source(ids), want)
    assert m.handle.get_counter("lstm_persist_fallbacks") == 2
    # sse_encode_score_topk reads the encoder's error flag together with the scores (one synchronisation per call): an id
    # out of range still raises, nothing is returned, and the next call is clean
    import sse_amd
    bad = ids.copy()
    bad[3, -1] = 300
    with pytest.raises(sse_amd.SSEError):
        m.handle.encode_score_topk(0, bad, False, 7)
    again_s, again_i = m.handle.encode_score_topk(0, ids, False, 7)
    assert np.array_equal(again_i, want_i) and np.array_equal(again_s, want_s)
    # back-off (option, off by default since the cluster kernels are launched cooperatively): after a launch that gave up
    # the following calls do not try the cluster kernel -- a time-out costs 10 ms -- and then it is tried again
    m.handle.set_option("lstm_cluster_backoff", 3)
    m.handle.set_option("lstm_persist_inject_miss", 1)
    assert np.array_equal(m.encode_source(ids), want)
    assert m.handle.get_counter("lstm_persist_fallbacks") == 3
    for _ in range(3):                                          # skipped: no launch, no (injected) miss, same bits
        assert np.array_equal(m.encode_source(ids), want)
    assert m.handle.get_counter("lstm_persist_fallbacks") == 3
    assert np.array_equal(m.encode_source(ids), want)           # tried again (and "misses" again)
    assert m.handle.get_counter("lstm_persist_fallbacks") == 4
    m.handle.set_option("lstm_persist_inject_miss", 0)
    m.handle.set_option("lstm_cluster_backoff", 0)


@pytest.mark.parametrize("H,S", [(40, 16), (100, 64), (72, 24)])
def test_cluster_kernel_with_workgroups_that_own_no_hidden_unit(H, S):
    """H = 40 on 16 workgroups leaves two of them without a unit: they skip the steps and pick h_T up for the
    projection; results stay bit-identical to the few-sequences kernel over many calls."""
    params = model_params("dual-encoder", 120, 20, H, H, S, 9)
    m, p = make_pair(params, seed=14)
    rng = np.random.RandomState(7)
    for it in range(20):
        ids = random_ids(rng, 1 + it % 7, 9, 120, 0.5)
        n0 = _paths(m.handle)
        got = m.encode_source(ids)
        _ran(m.handle, n0, lstm_path_persist=1, lstm_path_small=0)
        m.handle.set_option("lstm_persist_rows", 0)
        want = m.encode_source(ids)
        m.handle.set_option("lstm_persist_rows", 32)
        assert np.array_equal(got, want), it
    assert np.abs(got - O.encode(p, params, "src", ids)).max() <= TOL
    assert m.handle.get_counter("lstm_persist_fallbacks") == 0


def test_four_serving_handles_from_threads_while_a_fifth_trains():
    """sse_serving.py creates one handle per route: four handles issue single-query encode + score calls (the cluster
    kernel: 16 - 32 co-resident workgroups each) from four threads while a fifth handle runs train steps.  Every answer
    equals the quiet-machine answer, and (cooperative launches) none of them needed the fallback."""
    import threading
    params = model_params("dual-encoder", 400, 50, 96, 96, 64, 16)
    rng = np.random.RandomState(9)
    tgt = random_ids(rng, 571, 16, 400, 0.5)
    servers = []
    for _ in range(4):
        m, _p = make_pair(params, seed=21)
        m.handle.index_upload(m.encode_target(tgt).astype(np.float64))
        servers.append(m)
    queries = [random_ids(rng, 1, 16, 400, 0.5) for _ in range(12)]
    want = [servers[0].handle.encode_score_topk(0, q, False, 10) for q in queries]
    tparams = model_params("dual-encoder", 400, 50, 128, 128, 64, 16, lr=0.5)
    trainer, _p = make_pair(tparams, seed=22)
    tsrc = np.repeat(random_ids(rng, 128, 16, 400, 0.3), 2, axis=0)
    ttgt = random_ids(rng, 256, 16, 400, 0.3)
    tz = np.tile(np.array([1.0, 0.0], np.float32), 128)
    errs, stop = [], threading.Event()

    def train():
        try:
            while not stop.is_set():
                trainer.train_step(tsrc, ttgt, tz)
        except Exception as ex:                                 # pragma: no cover
            errs.append(ex)

    def serve(m):
        try:
            for _ in range(15):
                for q, (ws, wi) in zip(queries, want):
                    s, i = m.handle.encode_score_topk(0, q, False, 10)
                    assert np.array_equal(i, wi) and np.array_equal(s, ws)
        except Exception as ex:                                 # pragma: no cover
            errs.append(ex)

    tt = threading.Thread(target=train)
    tt.start()
    th = [threading.Thread(target=serve, args=(m,)) for m in servers]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    stop.set()
    tt.join(60)
    assert not errs, errs
    # the cluster kernels are launched cooperatively (hipLaunchCooperativeKernel): their workgroups are co-resident by the
    # runtime's promise, so no query of the four busy handles had to fall back to the few-sequences kernel
    assert sum(m.handle.get_counter("lstm_persist_fallbacks") for m in servers) == 0


@pytest.mark.parametrize("mode,V,E,Hs,Ht,S,T", [
    ("dual-encoder", 500, 50, 256, 256, 256, 32),          # configs[1]: 16 units per workgroup, two weight tiles
    ("shared-encoder", 300, 50, 96, 96, 64, 80),           # reference defaults: Hp = 128, 8 units per workgroup, 4 of 16 own only padding
    ("dual-encoder", 200, 40, 200, 130, 50, 50),           # crosslingual-like: padded cells, S not a multiple of 32
    ("dual-encoder", 90, 8, 16, 40, 512, 9),               # tiny cells, widest encoding (16 projection tiles)
])
def test_mfma_cluster_kernel_equals_the_other_kernels(mode, V, E, Hs, Ht, S, T):
    """lstm_cluster.hip (33 .. 1024 rows: hidden units of a 64-row tile over 16 workgroups, weights in LDS, h_t exchanged
    per step, gate GEMM on fp32 MFMA): bit-identical to the few-sequences kernel and to the matrix kernel, with and
    without the pad-prefix skip, for the evaluator's 600 and the index builder's 1000 rows and the ragged sizes around
    the 64-row clusters; within the encoder tolerance of the oracle."""
    params = model_params(mode, V, E, Hs, Ht, S, T)
    m, p = make_pair(params, seed=8)
    rng = np.random.RandomState(3)
    for B in (33, 64, 65, 600, 1000, 1024, 1025, 2100):        # (above 1024: two / three launches of the kernel)
        ids = random_ids(rng, B, T, V, pad_frac=0.6)
        ids[1, :] = 0
        ids[1, -1] = 1                                     # only EOS
        ids[2] = rng.randint(2, V, size=T)                 # no padding at all
        for side, enc in (("src", m.encode_source), ("tgt", m.encode_target)):
            for normalize in (True, False):
                m.handle.set_option("lstm_cluster_rows", 0)
                ref = enc(ids, normalize=normalize)                                   # few-sequences kernel
                m.handle.set_option("lstm_cluster_rows", 1024)
                n0 = _paths(m.handle)
                got = enc(ids, normalize=normalize)
                _ran(m.handle, n0, lstm_path_cluster=1, lstm_path_small=0, lstm_path_fwd=0)
                assert np.array_equal(got, ref), (B, side, normalize, np.abs(got - ref).max())
                # the any-placement publish path (write-through stores; taken when a cluster is not on one XCD)
                m.handle.set_option("lstm_cluster_write_through", 1)
                got_wt = enc(ids, normalize=normalize)
                m.handle.set_option("lstm_cluster_write_through", 0)
                _ran(m.handle, n0, lstm_path_cluster=2, lstm_path_small=0, lstm_path_fwd=0)
                assert np.array_equal(got_wt, ref), (B, side, normalize, "write-through")
            if B in (65, 600):
                m.handle.set_option("pad_skip", 0)
                got_noskip = enc(ids)
                m.handle.set_option("pad_skip", 1)
                assert np.array_equal(got_noskip, enc(ids))
        if B == 600:
            m.handle.set_option("lstm_small_rows", 0)
            m.handle.set_option("lstm_cluster_rows", 0)
            n0 = _paths(m.handle)
            mat = m.encode_source(ids)                                                # 32-row matrix tiles
            _ran(m.handle, n0, lstm_path_fwd=1, lstm_fwd_rows32=1, lstm_path_cluster=0)
            m.handle.set_option("lstm_small_rows", 1024)
            m.handle.set_option("lstm_cluster_rows", 1024)
            assert np.array_equal(m.encode_source(ids), mat)
        if B <= 65:
            assert np.abs(m.encode_source(ids) - O.encode(p, params, "src", ids)).max() <= TOL
    assert m.handle.get_counter("lstm_persist_fallbacks") == 0
    import sse_amd
    bad = random_ids(rng, 70, T, V)
    bad[69, -1] = V
    with pytest.raises(sse_amd.SSEError):
        m.encode_source(bad)
    good = random_ids(rng, 70, T, V)
    assert np.isfinite(m.encode_source(good)).all()
    # a missing cluster workgroup falls back to the few-sequences kernel
    m.handle.set_option("lstm_cluster_backoff", 0)
    m.handle.set_option("lstm_cluster_rows", 0)
    want = m.encode_source(good)
    m.handle.set_option("lstm_cluster_rows", 1024)
    m.handle.set_option("lstm_persist_inject_miss", 1)
    assert np.array_equal(m.encode_source(good), want)
    m.handle.set_option("lstm_persist_inject_miss", 0)
    assert m.handle.get_counter("lstm_persist_fallbacks") == 1
    # ... and for real: one workgroup of cluster 0 exits at once, the 15 others wait for its h.  The first wait gives up
    # after 10 ms, every other wait of the launch (all clusters, both groups, the projection's exchange) as soon as it
    # sees the error word: one time-out per launch, not one per step, then the few-sequences kernel.
    import time
    big = random_ids(rng, 600, T, V, pad_frac=0.3)
    m.handle.set_option("lstm_cluster_rows", 0)
    want = m.encode_source(big)
    m.handle.set_option("lstm_cluster_rows", 1024)
    m.handle.set_option("lstm_cluster_drop_wg", 1)
    t0 = time.perf_counter()
    got = m.encode_source(big)
    dt = time.perf_counter() - t0
    m.handle.set_option("lstm_cluster_drop_wg", 0)
    assert np.array_equal(got, want)
    assert m.handle.get_counter("lstm_persist_fallbacks") == 2
    assert dt < 0.25, dt
    assert np.array_equal(m.encode_source(big), want)          # and the next call is on the cluster kernel again
    assert m.handle.get_counter("lstm_persist_fallbacks") == 2


def test_mfma_cluster_kernel_many_calls_alternating_shapes():
    """Exchange buffers reused across calls (tag epochs), sides with different cell sizes, batch sizes on both sides of
    the 8-cluster launch boundary (512 rows)."""
    params = model_params("dual-encoder", 400, 50, 256, 96, 64, 16)
    m, p = make_pair(params, seed=23)
    rng = np.random.RandomState(8)
    cases = []
    for B, T in ((600, 16), (40, 16), (1024, 5), (513, 9), (100, 2)):
        ids = random_ids(rng, B, T, 400, pad_frac=0.4)
        m.handle.set_option("lstm_cluster_rows", 0)
        cases.append((ids, (m.encode_source(ids), m.encode_target(ids))))
    m.handle.set_option("lstm_cluster_rows", 1024)
    for it in range(300):
        ids, ref = cases[it % len(cases)]
        side = it % 2
        got = (m.encode_source if side == 0 else m.encode_target)(ids)
        if it % 23 == 0 or it > 290:
            assert np.array_equal(got, ref[side]), it


# --------------------------------------------------------------------------
# tf.nn.l2_normalize's clamp, x * rsqrt(max(sum(x^2), 1e-12)) (sse_model.py:282-283; SURVEY 4 "adversarial cases"):
# zero rows, rows whose squared norm is below the epsilon, denormal components -- through the exported
# sse_l2_normalize_dev and through every encoder kernel's fused normalise tail.
# --------------------------------------------------------------------------

def _clamp_rows(S, rng):
    x = rng.standard_normal((12, S)).astype(np.float32)
    x[0] = 0.0                                             # all-zero row: 0 * rsqrt(1e-12) = 0, not NaN
    x[1] *= np.float32(1e-8)                               # sum(x^2) ~ S * 1e-16 < 1e-12: clamp engaged, result = x * 1e6
    x[2] *= np.float32(1e-6) / np.float32(np.sqrt(S))      # squared norm ~ 1e-12: right at the epsilon
    x[3] = 0.0
    x[3, S // 2] = np.float32(1e-30)                       # square underflows to a denormal / zero
    x[4] = np.float32(1e-40)                               # denormal components throughout
    x[5] *= np.float32(3e-7)                               # just below the clamp
    x[6] *= np.float32(1e3)                                # ordinary rows on both sides of 1
    x[7, 1:] = 0.0
    return x


@pytest.mark.parametrize("S", [4, 64, 100, 256, 512])
def test_l2_normalize_dev_clamps_like_tf(S):
    """sse_l2_normalize_dev (exported entry, include/sse_hip.h) on zero / sub-epsilon / denormal rows == the oracle's
    tf.nn.l2_normalize restatement; zero rows stay exactly zero, nothing is NaN or inf."""
    import torch
    from tests.test_gpu_score import _scorer
    h = _scorer()
    x = _clamp_rows(S, np.random.RandomState(S))
    xd = torch.from_numpy(x).cuda()
    out = torch.full_like(xd, float("nan"))
    h.l2_normalize_dev(xd.data_ptr(), out.data_ptr(), x.shape[0], S)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), O.l2_normalize(x)
    assert np.all(np.isfinite(got))
    assert np.array_equal(got[0], np.zeros(S, np.float32))
    # clamp engaged: exactly x * rsqrt(1e-12) up to the rounding of the reciprocal square root
    assert np.allclose(got[1], x[1] * np.float32(1e6), rtol=2e-6, atol=0)
    assert np.abs(got - want).max() <= 2e-6 * max(1.0, float(np.abs(want).max()))
    nrm = np.linalg.norm(got[6:].astype(np.float64), axis=1)
    assert np.abs(nrm - 1).max() < 1e-6                    # ordinary rows come out unit length
    # in place (out == x) is what the in-graph predict path uses
    h.l2_normalize_dev(xd.data_ptr(), xd.data_ptr(), x.shape[0], S)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), got)


@pytest.mark.parametrize("B", [1, 40, 600, 1500, 9000])   # persist / cluster / cluster in chunks (or matrix) / matrix kernel, 64-row tiles
@pytest.mark.parametrize("scale", [0.0, 1e-9])
def test_encoder_normalise_tail_clamps_like_tf(B, scale):
    """An encoder whose projection is zero (raw encoding exactly 0) or tiny (squared norm of the raw encoding far below
    1e-12): the fused normalise tail of EVERY encoder kernel applies max(sum(x^2), 1e-12) like tf.nn.l2_normalize --
    zeros stay zeros, tiny rows come out as raw * 1e6, and the kernels agree bit for bit."""
    params = model_params("dual-encoder", 300, 50, 96, 96, 64, 12)
    m, p = make_pair(params, seed=9)
    p = dict(p)
    p["source_encoder/src_M"] = (p["source_encoder/src_M"] * np.float32(scale)).astype(np.float32)
    m.set_variables(p)
    rng = np.random.RandomState(B)
    ids = random_ids(rng, B, 12, 300, pad_frac=0.5)
    got = m.encode_source(ids)
    raw = m.encode_source(ids, normalize=False)
    assert np.all(np.isfinite(got))
    if scale == 0.0:
        assert not got.any() and not raw.any()
    else:
        assert 0 < np.abs(raw).max() < 1e-7                # sum of squares << 1e-12: clamp engaged on every row
        assert np.allclose(got, raw * np.float32(1e6), rtol=2e-6, atol=0)
        want = O.encode(p, params, "src", ids[:200])
        assert np.abs(got[:200] - want).max() <= 1e-4 * max(1.0, float(np.abs(want).max()))
    # the same rows through the few-sequences kernel (what every other kernel is bit-identical to)
    m.handle.set_option("lstm_persist_rows", 0)
    m.handle.set_option("lstm_cluster_rows", 0)
    n = min(B, 64)
    assert np.array_equal(m.encode_source(ids[:n]), got[:n])


def test_single_query_with_odd_pad_prefix_never_gives_up():
    """the single-query cluster kernel published its XCC-id handshake in the even exchange buffer, which a query
    with an ODD number of leading PADs overwrites in its first step.  Left-padded queries of every prefix length, many
    calls each: results equal the few-sequences kernel's and no launch falls back."""
    params = model_params("dual-encoder", 200, 50, 256, 256, 64, 16)
    m, p = make_pair(params, seed=12)
    rng = np.random.RandomState(0)
    before = m.handle.get_counter("lstm_persist_fallbacks")
    for npad in range(0, 15):
        ids = random_ids(rng, 3, 16, 200)
        ids[:, :npad] = 0
        n0 = _paths(m.handle)
        first = m.encode_source(ids)
        for _ in range(20):
            assert np.array_equal(m.encode_source(ids), first)
        _ran(m.handle, n0, lstm_path_persist=21, lstm_path_small=0)
        m.handle.set_option("lstm_persist_rows", 0)
        m.handle.set_option("lstm_cluster_rows", 0)
        assert np.array_equal(m.encode_source(ids), first)
        m.handle.set_option("lstm_persist_rows", 32)
        m.handle.set_option("lstm_cluster_rows", 1024)
    assert m.handle.get_counter("lstm_persist_fallbacks") == before


@pytest.mark.parametrize("H", [96, 64, 40, 72])
def test_small_cells_at_64_row_tiles_are_bit_identical_to_the_other_kernels(H):
    """H <= 96 at 64-row tiles (batches above 8192 rows): two or three live unit blocks, the third split by pass over two
    waves.  A row's result must not change a bit: against the few-sequences kernel (what every encoder kernel is
    bit-identical to), rows taken from everywhere in a 9,000-row batch, with and without the left-pad prefix skip."""
    params = model_params("dual-encoder", 400, 50, H, H, 64, 20)
    m, p = make_pair(params, seed=19)
    rng = np.random.RandomState(23)
    ids = random_ids(rng, 9000, 20, 400, pad_frac=0.6)
    for pad_skip in (1, 0):
        m.handle.set_option("pad_skip", pad_skip)
        n0 = _paths(m.handle)
        big = m.encode_source(ids)
        if pad_skip:          # (the host entry sorts this padded batch by prefix and then asks for 32-row tiles: padded_hint)
            _ran(m.handle, n0, lstm_path_fwd=1)
        else:
            _ran(m.handle, n0, lstm_path_fwd=1, lstm_fwd_rows64=1, lstm_fwd_gate_split=1)
        assert np.abs(big[:300] - O.encode(p, params, "src", ids[:300])).max() <= TOL
        pick = np.concatenate([np.arange(0, 40), np.arange(4480, 4520), np.arange(8960, 9000)])
        m.handle.set_option("lstm_persist_rows", 0)
        m.handle.set_option("lstm_cluster_rows", 0)
        small = m.encode_source(ids[pick])                   # 120 rows: the few-sequences kernel
        m.handle.set_option("lstm_persist_rows", 32)
        m.handle.set_option("lstm_cluster_rows", 1024)
        assert np.array_equal(big[pick], small)
    m.handle.set_option("pad_skip", 1)


@pytest.mark.parametrize("T,B,H,x3", [(50, 3000, 256, 0), (40, 1500, 96, 0), (130, 2100, 128, 0), (50, 2500, 256, 1)])
def test_device_pad_prefix_bucketing_is_bit_identical_in_caller_order(T, B, H, x3):
    """sse_encode_dev on left-padded rows (sse_index.py:79-85) already in HBM: the rows are bucketed by leading-PAD count on
    the device (pack.hip, option pad_sort_dev) as sse_encode does on the host; outputs stay in the caller's row order and equal
    the unbucketed run bit for bit.  Adaptive mode: the first call buckets (nothing seen yet), a dense batch switches the
    bucketing off for the following call, a padded one switches it on again -- results identical throughout."""
    import torch
    params = model_params("dual-encoder", 400, 50, H, H, 64, T)
    m, p = make_pair(params, seed=9)
    h = m.handle
    h.set_option("lstm_small_rows", 0)                   # the matrix kernel at every size
    h.set_option("lstm_cluster_rows", 0)
    h.set_option("lstm_x3", x3)
    rng = np.random.RandomState(T + B)
    ids = random_ids(rng, B, T, 400, pad_frac=0.98)
    ids[5, :] = 0                                        # all PAD (lead = T)
    ids[6, :] = rng.randint(2, 400, size=T)              # no padding
    ids[9, :-1] = 0                                      # only EOS
    ids[9, -1] = 1
    dense = random_ids(rng, B, T, 400)
    dev = torch.device("cuda", 0)
    out = torch.empty((B, 64), dtype=torch.float32, device=dev)

    def run(a, sort, skip=1):
        h.set_option("pad_skip", skip)
        h.set_option("pad_sort_dev", sort)
        d = torch.from_numpy(a).to(dev)
        h.encode_dev(0, d.data_ptr(), B, T, True, out.data_ptr())
        h.synchronize()
        return out.cpu().numpy().copy()

    want = run(ids, 0)
    assert np.array_equal(want, run(ids, 0, skip=0))
    n0 = h.get_counter("pad_sorted_calls")
    assert np.array_equal(run(ids, 2), want)             # always bucket, 32-row tiles
    assert h.get_counter("pad_sorted_calls") == n0 + 1
    want_dense = run(dense, 0)
    assert np.array_equal(run(dense, 2), want_dense)     # a dense batch through the bucketing: one bucket, same results
    n0 = h.get_counter("pad_sorted_calls")
    assert np.array_equal(run(ids, 1), want)             # adaptive: last completed call saw a dense batch -> class 0 ...
    assert np.array_equal(run(ids, 1), want)             # ... this one saw padding -> bucketed from here on
    assert np.array_equal(run(dense, 1), want_dense)
    assert np.array_equal(run(dense, 1), want_dense)     # not bucketed any more
    assert np.array_equal(run(ids, 1), want)
    assert h.get_counter("pad_sorted_calls") == n0 + 2   # calls 2 and 3 of the five
    if not x3:
        tol = TOL
        assert np.abs(want[:64] - O.encode(p, params, "src", ids[:64])).max() <= tol
    h.set_option("pad_skip", 1)
    h.set_option("pad_sort_dev", 1)


@pytest.mark.parametrize("H,S,T,B", [(96, 64, 24, 9000), (64, 64, 20, 8300), (128, 128, 16, 8500), (40, 50, 12, 8200),
                                     (100, 64, 9, 8193), (17, 40, 30, 8400), (96, 300, 10, 8257)])
def test_gate_split_kernel_is_bit_identical_to_the_unit_block_kernel(H, S, T, B):
    """lstm_fwd_gs.hip (small cells at 64-row tiles: one gate per wave, two phase-shifted row groups, no workgroup barrier in
    the time loop) against lstm_fwd_kernel<2,1,1> (option lstm_gate_split = 0): every bit equal -- dense and left-padded rows,
    with and without the prefix skip, a ragged last tile, both encoders (dual: separate weights), against the oracle too."""
    import torch
    params = model_params("dual-encoder", 400, 50, H, H, S, T)
    m, p = make_pair(params, seed=31)
    h = m.handle
    h.set_option("lstm_small_rows", 0)
    h.set_option("lstm_cluster_rows", 0)
    h.set_option("pad_sort_dev", 0)                     # caller order, 64-row tiles
    rng = np.random.RandomState(H + T)
    ids = random_ids(rng, B, T, 400, pad_frac=0.7)
    ids[:64] = random_ids(rng, 64, T, 400)               # one dense tile
    ids[70, :] = 0                                       # an all-PAD row
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(ids).to(dev)
    out = torch.empty((B, S), dtype=torch.float32, device=dev)
    res = {}
    for side in (0, 1):
        for skip in (1, 0):
            h.set_option("pad_skip", skip)
            for gs in (1, 0):
                h.set_option("lstm_gate_split", gs)
                for norm in (True, False):
                    out.zero_()
                    n0 = _paths(h)
                    h.encode_dev(side, d.data_ptr(), B, T, norm, out.data_ptr())
                    h.synchronize()
                    _ran(h, n0, lstm_path_fwd=1, lstm_fwd_rows64=1, lstm_fwd_gate_split=gs)
                    res[(side, skip, gs, norm)] = out.cpu().numpy().copy()
            for norm in (True, False):
                assert np.array_equal(res[(side, skip, 1, norm)], res[(side, skip, 0, norm)]), (side, skip, norm)
        assert np.array_equal(res[(side, 1, 1, True)], res[(side, 0, 1, True)])
        want = O.encode(p, params, "src" if side == 0 else "tgt", ids[:200])
        assert np.abs(res[(side, 1, 1, True)][:200] - want).max() <= TOL
    h.set_option("pad_skip", 1)
    h.set_option("lstm_gate_split", 1)
    h.set_option("pad_sort_dev", 1)
