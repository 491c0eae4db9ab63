"""CPU self-test of the raw-gradient comparison of tests/test_gpu_train_grads.py: keeps its bars honest.

At every case the GPU test runs, the float32 oracle must pass against the float64 oracle with 10x margin below each bar --
room for the device's different summation orders.  And backward defects that the weight / slot comparisons of the other
training tests cannot see (a first Adagrad step moves a weight by ~2.85 g, so their 2e-4 hides any gradient error below
~7e-5 absolute) must fail the comparison at the exact-fp32 bar, the bf16-rounded dG also at the split-bf16 bar.  The
defects go into a test-local restatement of oracle._lstm_backward, monkeypatched in; the oracle itself is not changed."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.test_gpu_train_grads import CASES, case_batch, case_params, cnn_min_pool_gap
from tests.util import (GRAD_BARS_EXACT, GRAD_BARS_SPLIT, LOSS_REL_EXACT, LOSS_REL_SPLIT, check_grads, check_tail,
                        oracle_float64, reference_grads)


def _inputs(c):
    params, p = case_params(c)
    src, tgt, z = case_batch(c)
    return params, p, src, tgt, z, c["rows_factor"] * len(z), bool(c["opts"].get("cnn_bf16"))


@pytest.mark.parametrize("c", CASES)
def test_float32_oracle_passes_every_bar_with_10x_margin(c):
    params, p, src, tgt, z, rows_global, bf16 = _inputs(c)
    if c["mode"] == "source_only_cnn":
        assert cnn_min_pool_gap(p, src, bf16) > 1e-5          # the GPU test's precondition: no near-tie in any max-pool
    bars = GRAD_BARS_SPLIT if c["split"] else GRAD_BARS_EXACT
    want, want_tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16)
    got, tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16, float64=False)
    assert O.F32 is np.float32 and O.FORGET_BIAS.dtype == np.float32          # the float64 switch did not leak
    margin = (bars[0] / 10, bars[1] / 10)
    check_grads(got, want, margin)
    check_tail(tail, want_tail, margin, (LOSS_REL_SPLIT if c["opts"].get("train_fwd_x3") else LOSS_REL_EXACT) / 10)


def test_oracle_float64_restores_the_float32_oracle_on_error():
    with pytest.raises(ZeroDivisionError):
        with oracle_float64():
            assert O.F32 is np.float64 and O.LOGIT_SCALE.dtype == np.float64
            1 / 0
    assert O.F32 is np.float32
    for name in ("FORGET_BIAS", "L2_EPS", "LOGIT_SCALE", "MAX_GRAD_NORM", "ADAGRAD_INIT_ACC"):
        assert getattr(O, name).dtype == np.float32, name


def _bptt(defect):
    """oracle._lstm_backward restated, with one defect switched in."""
    def backward(kernel, tape, dh_last, E):
        F32 = O.F32
        H = kernel.shape[1] // 4
        T = len(tape)
        B = dh_last.shape[0]
        dK = np.zeros_like(kernel)
        db = np.zeros(4 * H, F32)
        dX = np.zeros((B, T, E), F32)
        dh, dc = dh_last.astype(F32), np.zeros((B, H), F32)
        for t in range(T - 1, -1, -1):
            a, c_prev, si, sf, so, tj, tc = tape[t]
            do = dh * tc
            dc = dc + dh * so * (F32(1.0) - tc * tc)
            di, dj, df = dc * tj, dc * si, dc * c_prev
            dg = np.concatenate([di * si * (F32(1.0) - si), dj * (F32(1.0) - tj * tj),
                                 df * sf * (F32(1.0) - sf), do * so * (F32(1.0) - so)], axis=1).astype(F32)
            if defect == "dg_bf16":                  # a split operand that lost its lo half
                dg = O.bf16_round(dg)
            if not (defect == "dk_db_without_t0" and t == 0):
                dK += a.T @ dg
                db += dg.sum(axis=0, dtype=F32)
            da = dg @ kernel.T
            if not (defect == "dx_without_t0" and t == 0):
                dX[:, t, :] = da[:, :E]
            dh = da[:, E:].astype(F32)
            dc = (dc * sf).astype(F32)
        if defect == "forget_bias_x1.001":
            db[2 * H:3 * H] *= F32(1.001)
        return dK, db, dX
    return backward


def _case(cid):
    return next(c.values[0] for c in CASES if c.id == cid)


def test_restatement_without_defect_is_the_oracle(monkeypatch):
    params, p, src, tgt, z, rows_global, _ = _inputs(_case("shared96-s50"))
    want, want_tail = reference_grads(p, params, src, tgt, z, rows_global, float64=False)
    monkeypatch.setattr(O, "_lstm_backward", _bptt(None))
    got, tail = reference_grads(p, params, src, tgt, z, rows_global, float64=False)
    assert np.array_equal(tail, want_tail)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("defect,cid,bars,hits", [
    ("dg_bf16", "c1-paired", GRAD_BARS_EXACT, "kernel"),
    ("dg_bf16", "c1-paired", GRAD_BARS_SPLIT, "kernel"),
    ("dk_db_without_t0", "shared96-s50", GRAD_BARS_EXACT, "shared_encoder/rnn/basic_lstm_cell/kernel"),
    ("forget_bias_x1.001", "c1-paired", GRAD_BARS_EXACT, "bias"),
    ("forget_bias_x1.001", "x3-111", GRAD_BARS_EXACT, "bias"),
    ("dx_without_t0", "e32", GRAD_BARS_EXACT, "word_embedding"),
])
def test_backward_defects_are_rejected(monkeypatch, defect, cid, bars, hits):
    c = _case(cid)
    params, p, src, tgt, z, rows_global, _ = _inputs(c)
    want, _ = reference_grads(p, params, src, tgt, z, rows_global)
    monkeypatch.setattr(O, "_lstm_backward", _bptt(defect))
    got, _ = reference_grads(p, params, src, tgt, z, rows_global, float64=False)
    with pytest.raises(AssertionError, match=hits):
        check_grads(got, want, bars)


@pytest.mark.parametrize("cid", ["c1-paired", "seo-h128", "cnn"])
def test_tail_sum_of_squares_over_deduplicated_rows_is_rejected(cid):
    """tf.clip_by_global_norm takes the norm of the raw IndexedSlices values; summing the squares of the deduplicated
    (dense) rows instead is a different number wherever an id repeats in the batch."""
    c = _case(cid)
    params, p, src, tgt, z, rows_global, bf16 = _inputs(c)
    want, want_tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16)
    got, tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16, float64=False)
    check_tail(tail, want_tail, GRAD_BARS_EXACT, LOSS_REL_EXACT)
    dedup = tail.copy()
    dedup[0] = sum(float(np.sum(np.square(got[n].astype(np.float64))))
                   for n in ("word_embedding", "target_embedding/tgt_seq_embedding") if n in got)
    with pytest.raises(AssertionError, match=r"tail\[0\]"):
        check_tail(dedup, want_tail, GRAD_BARS_EXACT, LOSS_REL_EXACT)
