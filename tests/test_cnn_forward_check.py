"""CPU self-test of the forward comparison of tests/test_gpu_cnn_paths.py: keeps its bars honest.

On every case of its list, in both precisions and for normalised and raw encodings, the float32 oracle must be 10x inside
the bar against the float64 oracle (room for the device's summation orders and its split-operand projection), and the
tile-boundary preconditions must hold.  And forward defects of the kind a tiled kernel makes -- a position dropped at the end
or past a tile, half a k-group dropped, the bias on the wrong side of the ReLU, one operand left unrounded -- must exceed the
bar on these inputs.  The defects go into a test-local restatement of oracle.cnn_forward, monkeypatched in; the oracle itself
is not changed."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.test_gpu_cnn_paths import (FORWARD_CASES, boundary_misses, check_encoding, forward_case, reference_encode, rounded)
from tests.util import oracle_float64

CASE_PARAMS = [pytest.param(c, id=c["id"]) for c in FORWARD_CASES]


def _case(cid):
    return next(c for c in FORWARD_CASES if c["id"] == cid)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", CASE_PARAMS)
def test_float32_oracle_passes_the_forward_bars_with_10x_margin(c, bf16):
    params, p, ids = forward_case(c)
    assert len(ids) >= c["B"]
    for normalize in (True, False):
        want = reference_encode(p, params, ids, normalize, bf16)
        assert want.dtype == np.float64 and O.F32 is np.float32
        got = reference_encode(p, params, ids, normalize, bf16, float64=False)
        check_encoding(got, want, normalize, "%s: " % c["id"], margin=10.0)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in FORWARD_CASES if c["T"] >= 33 and c.get("kind") is None])
def test_every_tile_boundary_position_wins_somewhere(c, bf16):
    params, p, ids = forward_case(c)
    pp = rounded(p) if bf16 else p
    assert boundary_misses(pp, ids) == []
    with oracle_float64():
        assert boundary_misses({k: np.asarray(v, np.float64) for k, v in pp.items()}, ids) == []


def test_the_data_cases_hold_what_they_are_for():
    params, p, ids = forward_case(_case("pads"))
    assert not ids[0].any() and len(set(ids[2])) == 1 and np.array_equal(ids[4], ids[5]) and np.array_equal(ids[4], ids[-1])
    params, p, ids = forward_case(_case("dead"))
    for pp in (p, rounded(p)):
        pool = O.cnn_forward(pp, ids)
        assert 0.2 < np.mean(pool == 0) < 0.8 and not pool[3].any() and pool[0].any()
        assert pool[pool > 0].min() > 1e-5
    for normalize in (True, False):
        assert not reference_encode(p, params, ids, normalize, False)[3].any()
    shapes = {k: sorted(set(c[k] for c in FORWARD_CASES)) for k in "TESB"}
    assert set((5, 31, 32, 33, 36, 64, 68, 96, 150)) <= set(shapes["T"])
    assert set((1, 3, 4, 7, 50, 60, 63, 64)) <= set(shapes["E"])
    assert set((4, 50, 100, 512)) <= set(shapes["S"])
    assert set((1, 7, 8, 9, 33, 1093)) <= set(shapes["B"])


def _forward(defect):
    """oracle.cnn_forward restated, with one defect switched in."""
    def cnn_forward(params, ids, keep_tape=False, bf16=False):
        F32 = O.F32
        emb = params["word_embedding"]
        ids = O.check_ids(ids, emb.shape[0])
        B, T = ids.shape
        E = emb.shape[1]
        x = emb[ids]
        if bf16 and defect != "bf16_embeddings_unrounded":
            x = O.bf16_round(x)
        feats, tape = [], []
        for fs, nf in zip(O.CNN_FILTER_SIZES, O.CNN_NUM_FILTERS):
            W = params["source_only_cnn/conv-maxpool-%d/W" % fs].reshape(-1, nf)
            if bf16:
                W = O.bf16_round(W)
            b = params["source_only_cnn/conv-maxpool-%d/b" % fs]
            P = T - fs + 1
            Ep = (E + 3) // 4 * 4
            if defect == "half_k_group_dropped" and fs * Ep % 8 == 4:      # k' = d * Ep + e in [fs * Ep - 4, fs * Ep)
                W = W.copy()
                W.reshape(fs, E, nf)[fs - 1, max(0, Ep - 4):, :] = 0
            win = np.stack([x[:, q:q + fs, :].reshape(B, -1) for q in range(P)], axis=1)
            conv = np.stack([win[:, q, :] @ W for q in range(P)], axis=1)
            if defect == "bias_after_relu":
                hconv = np.maximum(conv, F32(0.0)) + b
            else:
                hconv = np.maximum(conv + b, F32(0.0))
            if defect == "last_position_of_width_3_dropped" and fs == 3:
                hconv = hconv[:, :P - 1]
            if defect == "width_5_positions_from_32_dropped" and fs == 5:
                hconv = hconv[:, :32]
            feats.append(hconv.max(axis=1))
            if keep_tape:
                tape.append((win, hconv))
        pool = np.concatenate(feats, axis=1).astype(F32)
        return (pool, tape) if keep_tape else pool
    return cnn_forward


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cid", ["t32-e4-b8", "t36-e60", "pads", "dead"])
def test_restatement_without_defect_is_the_oracle(monkeypatch, cid, bf16):
    params, p, ids = forward_case(_case(cid))
    want = [reference_encode(p, params, ids, n, bf16, float64=False) for n in (True, False)]
    pool, tape = O.cnn_forward(p, ids, keep_tape=True, bf16=bf16)
    monkeypatch.setattr(O, "cnn_forward", _forward(None))
    got = [reference_encode(p, params, ids, n, bf16, float64=False) for n in (True, False)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    pool2, tape2 = O.cnn_forward(p, ids, keep_tape=True, bf16=bf16)
    assert np.array_equal(pool, pool2) and all(np.array_equal(a[1], b[1]) for a, b in zip(tape, tape2))


@pytest.mark.parametrize("defect,bf16,cids", [
    ("last_position_of_width_3_dropped", False, ["t33-e7", "t36-e60", "t64-e50-s512", "t68-e63", "t96-e64", "t150-e50"]),
    ("last_position_of_width_3_dropped", True, ["t33-e7", "t96-e64", "t144-e64"]),
    ("width_5_positions_from_32_dropped", False, ["t64-e50-s512", "t68-e63", "t96-e64", "t150-e50"]),
    ("width_5_positions_from_32_dropped", True, ["t64-e50-s512", "t68-e63", "t144-e64"]),
    ("half_k_group_dropped", False, ["t32-e4-b8", "t36-e60"]),
    ("half_k_group_dropped", True, ["t32-e4-b8", "t36-e60"]),
    ("bias_after_relu", False, ["dead"]),         # (visible only where a pooled feature is 0: biases below 0)
    ("bias_after_relu", True, ["dead"]),
    ("bf16_embeddings_unrounded", True, ["t12-e7-b9", "t36-e60", "t96-e64", "scale-1e3"]),
])
def test_forward_defects_are_rejected(monkeypatch, defect, bf16, cids):
    """The float32 oracle with the defect, against the float64 oracle without: over the bar for normalised and for raw
    encodings, at each named case."""
    for cid in cids:
        params, p, ids = forward_case(_case(cid))
        want = {n: reference_encode(p, params, ids, n, bf16) for n in (True, False)}
        with monkeypatch.context() as mp:
            mp.setattr(O, "cnn_forward", _forward(defect))
            got = {n: reference_encode(p, params, ids, n, bf16, float64=False) for n in (True, False)}
        for n in (True, False):
            with pytest.raises(AssertionError, match="max\\|d\\|"):
                check_encoding(got[n], want[n], n, "%s: " % cid)
