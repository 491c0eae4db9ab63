"""Option lstm_x_table: the matrix encoder (Hp = 256 / 512) starts every step's gate accumulators from a per-token table of x
projections (csrc/lstm_xtable.hip) instead of recomputing them from the embedding row.  The table is built with the
recurrence's own MFMA chain, so every encoding must equal the embedding-gather path's bit for bit, and a weight change must
never leave a stale table behind."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import make_pair, model_params, random_ids

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _matrix_kernel_only(h):
    for opt in ("lstm_persist_rows", "lstm_cluster_rows", "lstm_small_rows"):
        h.set_option(opt, 0)


def _both(m, enc, ids, normalize):
    """(x-table path, embedding-gather path) encodings of one batch."""
    n = m.handle.get_counter("lstm_fwd_x_table")
    m.handle.set_option("lstm_x_table", 2)
    fast = enc(ids, normalize=normalize)
    assert m.handle.get_counter("lstm_fwd_x_table") == n + 1       # the matrix kernel's table path ran ...
    m.handle.set_option("lstm_x_table", 0)
    full = enc(ids, normalize=normalize)
    assert m.handle.get_counter("lstm_fwd_x_table") == n + 1       # ... and here its embedding gather
    m.handle.set_option("lstm_x_table", 1)
    return fast, full


CASES = [
    # mode, V, E, Hs, Ht, S, T, B
    ("dual-encoder", 500, 50, 256, 256, 256, 32, 9000),    # configs[1] shape at 64-row tiles (<2,2,1>)
    ("shared-encoder", 500, 50, 256, 256, 256, 32, 9000),  # one table for both sides
    ("dual-encoder", 300, 50, 256, 200, 128, 20, 1000),    # 32-row tiles (<1,1,1>), B not a multiple of 64, padding unit blocks
    ("dual-encoder", 200, 50, 512, 300, 128, 12, 333),     # Hp = 512 (<1,1,2>), 10 live unit blocks on the target side
    ("dual-encoder", 400, 40, 256, 512, 64, 1, 777),       # T = 1: no recurrent k-group at all
]


@pytest.mark.parametrize("pad", [0.0, 0.8])               # left padding: pad-prefix skip + host row sort (row_map)
@pytest.mark.parametrize("mode,V,E,Hs,Ht,S,T,B", CASES)
def test_x_table_is_bit_identical(mode, V, E, Hs, Ht, S, T, B, pad):
    params = model_params(mode, V, E, Hs, Ht, S, T)
    m, p = make_pair(params, seed=4)
    _matrix_kernel_only(m.handle)
    rng = np.random.RandomState(B + T)
    ids = random_ids(rng, B, T, V, pad_frac=pad)
    if pad:
        ids[3, :] = 0                                      # all PAD
    n0 = m.handle.get_counter("lstm_x_table_builds")
    for side, enc in (("src", m.encode_source), ("tgt", m.encode_target)):
        for normalize in (True, False):
            fast, full = _both(m, enc, ids, normalize)
            assert np.array_equal(fast, full), (side, normalize, float(np.abs(fast - full).max()))
        assert np.abs(fast[:24] - O.encode(p, params, side, ids[:24], normalize=False)).max() <= TOL * max(1.0, np.abs(full).max())
    # one table per LSTM owner, built once (no weight change in between)
    assert m.handle.get_counter("lstm_x_table_builds") - n0 == (1 if mode == "shared-encoder" else 2)


@pytest.mark.parametrize("sort", [0, 2])
def test_x_table_with_device_pad_sort(sort):
    import torch
    V, T, B = 400, 24, 3000
    params = model_params("dual-encoder", V, 50, 256, 256, 64, T)
    m, _ = make_pair(params, seed=8)
    h = m.handle
    _matrix_kernel_only(h)
    h.set_option("pad_sort_dev", sort)
    ids = random_ids(np.random.RandomState(5), B, T, V, pad_frac=0.98)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(ids).to(dev)
    out = torch.empty((B, 64), dtype=torch.float32, device=dev)
    got = {}
    for xt in (2, 0):
        h.set_option("lstm_x_table", xt)
        h.encode_dev(0, d.data_ptr(), B, T, True, out.data_ptr())
        h.synchronize()
        got[xt] = out.cpu().numpy().copy()
    assert np.array_equal(got[2], got[0])
    assert h.get_counter("lstm_x_table_builds") == 1


def test_x_table_out_of_range_id_sets_the_same_error():
    import sse_amd
    V, T = 300, 16
    params = model_params("dual-encoder", V, 50, 256, 256, 64, T)
    m, _ = make_pair(params, seed=2)
    _matrix_kernel_only(m.handle)
    ids = random_ids(np.random.RandomState(1), 700, T, V, pad_frac=0.5)
    good = ids.copy()
    for bad in (V, -1):
        ids[611, T - 3] = bad
        for xt in (2, 0):
            m.handle.set_option("lstm_x_table", xt)
            with pytest.raises(sse_amd.SSEError):
                m.encode_source(ids)
            ok = m.encode_source(good)                     # the handle stays usable
            assert np.isfinite(ok).all()
    fast, full = _both(m, m.encode_source, good, True)
    assert np.array_equal(fast, full)


def test_x_table_follows_weight_changes():
    """A train step and set_variables both invalidate the table: the next encode equals a fresh handle holding those weights
    on the embedding-gather path."""
    V, T, B = 300, 16, 2000
    params = model_params("dual-encoder", V, 50, 256, 256, 128, T)
    m, _ = make_pair(params, seed=6)
    _matrix_kernel_only(m.handle)
    m.handle.set_option("lstm_x_table", 2)
    rng = np.random.RandomState(7)
    ids = random_ids(rng, B, T, V, pad_frac=0.5)

    def fresh(weights):
        f, _ = make_pair(params, seed=6)
        _matrix_kernel_only(f.handle)
        f.handle.set_option("lstm_x_table", 0)
        f.set_variables(weights)
        return f

    m.encode_source(ids)
    m.encode_target(ids)
    n0 = m.handle.get_counter("lstm_x_table_builds")
    src = np.repeat(random_ids(rng, 32, T, V, 0.5), 2, axis=0)
    m.train_step(src, random_ids(rng, 64, T, V, 0.5), np.tile(np.array([1.0, 0.0], np.float32), 32))
    w = m.get_variables()
    f = fresh(w)
    assert np.array_equal(m.encode_source(ids), f.encode_source(ids))
    assert np.array_equal(m.encode_target(ids), f.encode_target(ids))
    assert m.handle.get_counter("lstm_x_table_builds") == n0 + 2

    w2 = dict(w)
    w2["word_embedding"] = (w["word_embedding"] * 0.9).astype(np.float32)
    m.set_variables({"word_embedding": w2["word_embedding"]})
    f = fresh(w2)
    assert np.array_equal(m.encode_source(ids), f.encode_source(ids))
    k = "source_encoder/rnn/basic_lstm_cell/kernel"
    w2[k] = (w[k] * 1.1).astype(np.float32)
    m.set_variables({k: w2[k]})
    f = fresh(w2)
    assert np.array_equal(m.encode_source(ids), f.encode_source(ids))


def test_x_table_build_policy_and_cap():
    V, T = 4000, 10
    params = model_params("dual-encoder", V, 50, 256, 256, 64, T)
    m, _ = make_pair(params, seed=3)
    h = m.handle
    _matrix_kernel_only(h)
    rng = np.random.RandomState(4)
    small = random_ids(rng, 350, T, V)                    # B * T < V: no build under the default policy
    big = random_ids(rng, 450, T, V)                      # B * T >= V: built
    h.set_option("lstm_x_table", 0)
    want_small, want_big = m.encode_source(small), m.encode_source(big)
    h.set_option("lstm_x_table", 1)
    assert np.array_equal(m.encode_source(small), want_small)
    assert h.get_counter("lstm_x_table_builds") == 0
    assert np.array_equal(m.encode_source(big), want_big)
    assert h.get_counter("lstm_x_table_builds") == 1
    assert np.array_equal(m.encode_source(small), want_small)   # a valid table serves any batch
    # a cap below the table's size (4000 tokens x 4 KiB = 15.6 MiB): the embedding-gather path, nothing built
    m.set_variables({"word_embedding": m.get_variables()["word_embedding"]})
    h.set_option("lstm_x_table_mb", 15)
    h.set_option("lstm_x_table", 2)
    assert np.array_equal(m.encode_source(big), want_big)
    assert h.get_counter("lstm_x_table_builds") == 1
    h.set_option("lstm_x_table_mb", 16)
    assert np.array_equal(m.encode_source(big), want_big)
    assert h.get_counter("lstm_x_table_builds") == 2
