"""The x-table path of the matrix encoder loads every pass's table fragments one pass ahead (pass B's under pass A's last
k-groups and epilogue, the next step's pass A under pass B's; `<2,2,1>`, 64-row tiles at Hp = 256).  Only the time at which
the same table values reach the accumulators changes, so every encoding must still equal the embedding-gather path
(lstm_x_table = 0) bit for bit: first and last steps, pad-prefix starts (t0 > 0 with a row map), partial tiles, both row
tiles and Hp = 512.  The ids of step t+1 are range-checked before their prefetch: a bad one must fail the encode exactly as
on the gather path."""
import numpy as np
import pytest

from tests.util import make_pair, model_params, random_ids

pytestmark = pytest.mark.gpu


def _matrix_kernel_only(h):
    for opt in ("lstm_persist_rows", "lstm_cluster_rows", "lstm_small_rows"):
        h.set_option(opt, 0)


def _model(V, H, T, S=64, seed=11):
    params = model_params("dual-encoder", V, 40, H, H, S, T)
    m, _ = make_pair(params, seed=seed)
    _matrix_kernel_only(m.handle)
    return m


def _encode_both(m, ids, side="src"):
    enc = m.encode_source if side == "src" else m.encode_target
    out = {}
    for xt in (2, 0):
        m.handle.set_option("lstm_x_table", xt)
        out[xt] = enc(ids, normalize=False)
    m.handle.set_option("lstm_x_table", 1)
    return out[2], out[0]


@pytest.mark.parametrize("rows", ["32", "64"])
@pytest.mark.parametrize("T", [1, 2, 32])
@pytest.mark.parametrize("B", [1, 45, 1093])               # one row, a partial tile, many tiles with a partial last one
def test_prefetch_matches_gather_path(monkeypatch, rows, T, B):
    monkeypatch.setenv("SSE_FWD_ROWS", rows)
    V = 300
    m = _model(V, 256, T)
    ids = random_ids(np.random.RandomState(B * 7 + T), B, T, V)
    for side in ("src", "tgt"):
        fast, full = _encode_both(m, ids, side)
        assert np.array_equal(fast, full), (side, float(np.abs(fast - full).max()))


@pytest.mark.parametrize("rows", ["32", "64"])
@pytest.mark.parametrize("sort", [0, 2])
def test_prefetch_with_pad_prefix_and_row_map(monkeypatch, rows, sort):
    """Left-padded rows: tiles start at t0 > 0 from the pad-prefix state, rows sorted by pad count (host or device sort)."""
    import torch
    monkeypatch.setenv("SSE_FWD_ROWS", rows)
    V, T, B = 400, 24, 1500
    m = _model(V, 256, T)
    h = m.handle
    h.set_option("pad_sort_dev", sort)
    ids = random_ids(np.random.RandomState(9), B, T, V, pad_frac=0.9)
    ids[:200, :T - 2] = 0                                  # a block of rows with only two real steps: whole tiles start late
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
    fast, full = _encode_both(m, ids)                      # host path (host row sort)
    assert np.array_equal(fast, full)


@pytest.mark.parametrize("H", [300, 512])
def test_prefetch_hp512(H):
    """Hp = 512 (<1,1,2>: two unit blocks per wave, padding blocks at H = 300) keeps the pass-head loads."""
    V, T, B = 250, 12, 333
    m = _model(V, H, T)
    ids = random_ids(np.random.RandomState(H), B, T, V, pad_frac=0.5)
    for side in ("src", "tgt"):
        fast, full = _encode_both(m, ids, side)
        assert np.array_equal(fast, full), side


@pytest.mark.parametrize("rows", ["32", "64"])
@pytest.mark.parametrize("where", ["second", "last", "after_pad"])
def test_bad_id_of_the_next_step_fails_like_the_gather_path(monkeypatch, rows, where):
    """An out-of-range id met only as step t+1's prefetch (never at the tile's first step) raises on both paths, and the
    handle stays usable."""
    import sse_amd
    monkeypatch.setenv("SSE_FWD_ROWS", rows)
    V, T, B = 300, 16, 700
    m = _model(V, 256, T)
    good = random_ids(np.random.RandomState(3), B, T, V)
    r = 517
    if where == "after_pad":
        good[r, :5] = 0
    col = {"second": 1, "last": T - 1, "after_pad": 6}[where]
    for bad in (V, -1):
        ids = good.copy()
        ids[r, col] = bad
        for xt in (2, 0):
            m.handle.set_option("lstm_x_table", xt)
            with pytest.raises(sse_amd.SSEError):
                m.encode_source(ids)
            assert np.isfinite(m.encode_source(good)).all()
    fast, full = _encode_both(m, good)
    assert np.array_equal(fast, full)
