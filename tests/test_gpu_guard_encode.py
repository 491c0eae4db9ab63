"""sse_encode_dev and sse_l2_normalize_dev on guarded, skewed caller buffers (tests/guard_bands.py): the id matrix [B][T] and
the encodings [B][S] sit between guards, with no skew and one element off 16-byte alignment, under both fills.

One case per kernel path, forced and proved by counter with the selectors of tests/test_gpu_lstm_paths.py, at the smallest
batch that crosses the path's tile edge; the text-CNN in both precisions with the cases of tests/test_gpu_cnn_paths.py.  The
references and bars are those files' (the oracle in float64 on the float32 parameters).  An encode's arithmetic cannot depend
on where its buffers lie, so every result must also be bit-identical to the same call on whole allocations -- except where
launch_l2_normalize (pack.hip) runs on the caller's rows: its 16-byte body and its scalar body sum a row in different orders,
so a skewed call with cols % 4 == 0 is held to its oracle bar alone.  That is sse_l2_normalize_dev (the bar of
tests/test_gpu_encode.py::test_l2_normalize_dev_clamps_like_tf), and inside sse_encode_dev the normalised any-shape path and
the normalised target side of a free target matrix (_l2_takes_another_body)."""
import functools

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import guard_bands as GB
from tests import test_gpu_cnn_paths as CP
from tests import test_gpu_lstm_paths as LP
from tests.util import model_params, oracle_params, random_ids

pytestmark = pytest.mark.gpu

_lc = LP._lc
# Every case goes through sse_encode_dev.  B on the tile edges of its kernel: 4 sequences x 8 clusters (persist), 64-row tiles
# (cluster, matrix kernel), 4 rows per workgroup (few-sequences); S = 50 and S = 64; the 64-row matrix tiles exist only above
# 8192 rows (lstm_fwd_rows_per_wg), so those three cases keep the shapes tests/test_gpu_lstm_paths.py gives them.
ENC_CASES = [
    _lc("persist-b1", "persist", 300, 50, 96, 64, 8, 1, pad=0.0), _lc("persist-b5-s50", "persist", 300, 50, 96, 50, 8, 5),
    _lc("cluster-b33-s50", "cluster", 300, 50, 128, 50, 8, 33),
    _lc("small-b7", "small", 300, 50, 96, 64, 8, 7), _lc("small-b5-s50", "small", 300, 50, 96, 50, 8, 5),
    _lc("fwd32-b65-s50", "fwd32", 300, 50, 96, 50, 8, 65), _lc("fwd32-b64", "fwd32", 300, 50, 128, 64, 8, 64),
    # left-padded ids, rows bucketed by prefix on the device: the scatter back to the caller's order is a store by a permuted index
    _lc("fwd32-pads-sorted", "fwd32", 300, 50, 96, 50, 12, 70, kind="pads", opts=dict(pad_sort_dev=2), pad_sorted=1),
    _lc("fwd64-gs-h96", "fwd64gs", 300, 50, 96, 64, 6, 8296), _lc("fwd64-h96", "fwd64", 300, 50, 96, 64, 6, 8296, opts=dict(lstm_gate_split=0)),
    _lc("xt32-h129", "xt32", 203, 50, 129, 64, 8, 70, kind="vmax"), _lc("xt64-h256", "xt64", 203, 50, 256, 64, 6, 8250, kind="vmax"),
    _lc("x3-h96-e50", "x3", 300, 50, 96, 50, 8, 70),
    _lc("generic-e400", "generic", 100, 400, 64, 64, 6, 9),
]


def _guard(rows, cols):
    return GB.guard_bytes(rows, cols, 4, 64, 64)


def _l2_takes_another_body(skew, cols):
    """launch_l2_normalize (pack.hip) on a pointer that is not 16-byte aligned takes its scalar body where the whole allocation takes
    the 16-byte one (cols % 4 == 0, cols <= 1024): the row's sum of squares in another order, so no bit-identity -- the oracle bar
    alone.  Reached by sse_l2_normalize_dev, and by sse_encode_dev where it normalises the caller's rows in place: the any-shape
    path and the target side of the modes whose target encoder is the free matrix."""
    return skew == 1 and cols % 4 == 0 and cols <= 1024


def _encode_specs(ids, S):
    B, T = ids.shape
    return dict(ids=GB.spec(np.int32, B * T, "in", init=ids, valid=2, guard=_guard(B, T)),          # 2: an in-range non-PAD token id
                out=GB.spec(np.float32, B * S, "out", guard=_guard(B, S)))


def _encode_call(h, side, B, T, normalize):
    def call(b):
        h.encode_dev(side, b["ids"].ptr, B, T, normalize, b["out"].ptr)
        h.synchronize()
    return call


@functools.lru_cache(maxsize=None)
def _lstm_setup(cid):
    c = next(c for c in ENC_CASES if c["id"] == cid)
    params, p, ids = LP.lstm_case(c)
    return c, params, p, ids, LP.reference_encodings(p, params, "src", ids)


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("cid", [c["id"] for c in ENC_CASES])
def test_lstm_encode_on_guarded_buffers(cid, skew):
    c, params, p, ids, want = _lstm_setup(cid)
    B, T, S = ids.shape[0], ids.shape[1], c["S"]
    m = LP._model(c, params, p)
    be = GB.TorchBackend()
    before, calls = LP._counters(m.handle), GB.run_guarded.calls
    for normalize in (True, False):
        GB.drive(be, _encode_specs(ids, S), _encode_call(m.handle, 0, B, T, normalize), skew,
                 lambda o: LP.check_encoding(o["out"].reshape(B, S), want[normalize], normalize, LP.bars_of(c), "%s skew %d: " % (cid, skew)),
                 identical=not (c["kernel"] == "generic" and normalize and _l2_takes_another_body(skew, S)))
    LP.assert_kernel_ran(c, before, LP._counters(m.handle), 6, "%s: " % cid)       # (whole allocations + two fills) x (normalised, raw)
    print("GUARDCALLS encode %d" % (GB.run_guarded.calls - calls))


@pytest.mark.parametrize("skew", (0, 1))
def test_cells_of_33_and_129_units_with_19_columns_on_guarded_buffers(skew):
    """Nothing a multiple of anything: source cell 33, target cell 129, S = 19, B = 37; both sides, whichever kernel serves them."""
    params = model_params("dual-encoder", 90, 9, 33, 129, 19, 7)
    p = oracle_params(params, seed=11)
    ids = random_ids(np.random.RandomState(12), 37, 7, 90, pad_frac=0.5)
    import sse_amd
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    be = GB.TorchBackend()
    calls = GB.run_guarded.calls
    for side, name in ((0, "src"), (1, "tgt")):
        want = LP.reference_encodings(p, params, name, ids)
        for normalize in (True, False):
            GB.drive(be, _encode_specs(ids, 19), _encode_call(m.handle, side, 37, 7, normalize), skew,
                     lambda o: LP.check_encoding(o["out"].reshape(37, 19), want[normalize], normalize, LP.BARS_EXACT, "%s: " % name))
    print("GUARDCALLS encode %d" % (GB.run_guarded.calls - calls))


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("S", (50, 64))
def test_target_side_of_a_free_target_matrix_on_guarded_buffers(S, skew):
    """source-encoder-only: the target "encoder" is the [N][S] matrix itself -- normalised through launch_l2_normalize into the
    caller's rows, or copied raw; the ids are not read."""
    N, T = 17, 6
    params = model_params("source-encoder-only", 60, 8, 32, 32, S, T, N=N)
    p = oracle_params(params, seed=5)
    import sse_amd
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    table = np.asarray(p["target_embedding/tgt_seq_embedding"], np.float32).reshape(N, S)
    ids = random_ids(np.random.RandomState(6), N, T, 60)
    calls = GB.run_guarded.calls
    for normalize in (True, False):
        want = O.l2_normalize(table) if normalize else table

        def check(o):
            got = o["out"].reshape(N, S)
            if normalize:
                assert np.abs(got - want).max() <= 2e-6 * max(1.0, float(np.abs(want).max()))     # the bar of sse_l2_normalize_dev
            else:
                assert GB.same_bits(got, want)
        GB.drive(GB.TorchBackend(), _encode_specs(ids, S), _encode_call(m.handle, 1, N, T, normalize), skew, check,
                 identical=not (normalize and _l2_takes_another_body(skew, S)))
    print("GUARDCALLS encode %d" % (GB.run_guarded.calls - calls))


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cid", ["t12-e7-b9", "t20-e24-b33"])          # S = 50 with 9 rows; S = 64 with one row into a second tile
def test_cnn_encode_on_guarded_buffers(cid, bf16, skew):
    c = next(c for c in CP.FORWARD_CASES if c["id"] == cid)
    params, p, ids = CP.forward_case(c)
    B, T, S = ids.shape[0], ids.shape[1], c["S"]
    m = CP._model(params, p, bf16)
    be = GB.TorchBackend()
    calls = GB.run_guarded.calls
    for normalize in (True, False):
        want = CP.reference_encode(p, params, ids, normalize, bf16)
        GB.drive(be, _encode_specs(ids, S), _encode_call(m.handle, 0, B, T, normalize), skew,
                 lambda o: CP.check_encoding(o["out"].reshape(B, S), want, normalize, "%s skew %d: " % (cid, skew)))
    print("GUARDCALLS encode %d" % (GB.run_guarded.calls - calls))


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("cols", (3, 50, 64, 260, 1028))               # 1028: a multiple of 4 above the 16-byte body's 1024
@pytest.mark.parametrize("rows", (1, 7, 65))
def test_l2_normalize_on_guarded_buffers(rows, cols, skew):
    from tests.test_gpu_score import _scorer
    h = _scorer()
    rng = np.random.RandomState(rows * 2000 + cols)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    x[0] *= np.float32(1e-9)                                           # below the clamp: x * 1e6
    if rows > 2:
        x[2] = 0.0
    want = O.l2_normalize(x)
    specs = dict(x=GB.spec(np.float32, rows * cols, "in", init=x, guard=_guard(rows, cols)),
                 out=GB.spec(np.float32, rows * cols, "out", guard=_guard(rows, cols)))

    def call(b):
        h.l2_normalize_dev(b["x"].ptr, b["out"].ptr, rows, cols)

    def check(o):
        got = o["out"].reshape(rows, cols)
        assert np.isfinite(got).all() and (rows <= 2 or not got[2].any())
        assert np.abs(got - want).max() <= 2e-6 * max(1.0, float(np.abs(want).max()))
    calls = GB.run_guarded.calls
    GB.drive(GB.TorchBackend(), specs, call, skew, check, identical=not _l2_takes_another_body(skew, cols))
    print("GUARDCALLS encode %d" % (GB.run_guarded.calls - calls))
    h.close()
