"""CPU self-test of the raw-gradient comparison of tests/test_gpu_train_grads.py: keeps its bars honest.

At every case the GPU test runs, the float32 oracle must pass against the float64 oracle with 10x margin below each bar --
room for the device's different summation orders.  And backward defects that the weight / slot comparisons of the other
training tests cannot see (a first Adagrad step moves a weight by ~2.85 g, so their 2e-4 hides any gradient error below
~7e-5 absolute) must fail the comparison at the exact-fp32 bar, the bf16-rounded dG also at the split-bf16 bar.  The
defects go into test-local restatements of oracle._lstm_backward and oracle._cnn_gradients, monkeypatched in; the oracle
itself is not changed."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.test_gpu_train_grads import CASES, case_bars, case_batch, case_params, cnn_preconditions
from tests.util import (GRAD_BARS_EXACT, GRAD_BARS_SPLIT, LOSS_REL_EXACT, LOSS_REL_SPLIT, check_grads, check_tail,
                        oracle_float64, reference_grads)


def _inputs(c):
    params, p = case_params(c)
    src, tgt, z = case_batch(c)
    return params, p, src, tgt, z, c["rows_factor"] * len(z), bool(c["opts"].get("cnn_bf16"))


@pytest.mark.parametrize("c", CASES)
def test_float32_oracle_passes_every_bar_with_10x_margin(c):
    params, p, src, tgt, z, rows_global, bf16 = _inputs(c)
    cnn_preconditions(c, p, src)          # the GPU test's preconditions: no max-pool near a tie, no pooled feature near 0
    bars = case_bars(c)
    assert bars[0] <= GRAD_BARS_SPLIT[0] and bars[1] <= GRAD_BARS_SPLIT[1]
    for vb in (c.get("var_bars") or {}).values():             # a variable's own bar is never the tighter one to pass here
        assert GRAD_BARS_EXACT[0] <= vb[0] <= GRAD_BARS_SPLIT[0] and GRAD_BARS_EXACT[1] <= vb[1] <= GRAD_BARS_SPLIT[1]
    want, want_tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16)
    got, tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16, float64=False)
    assert O.F32 is np.float32 and O.FORGET_BIAS.dtype == np.float32          # the float64 switch did not leak
    margin = (bars[0] / 10, bars[1] / 10)
    check_grads(got, want, margin)
    check_tail(tail, want_tail, margin, (LOSS_REL_SPLIT if c["opts"].get("train_fwd_x3") else LOSS_REL_EXACT) / 10)


def test_small_preactivation_case_is_as_small_as_intended():
    """Zero LSTM biases and an embedding of +-2.5e-3: every cell state, hence every argument of the cell-output tanh, stays
    below 1e-2 -- deep inside the range where the fused kernels' tanh is a polynomial -- and the gradients are not all zero."""
    c = next(c.values[0] for c in CASES if c.id == "small-preactivations")
    params, p = case_params(c)
    src, tgt, z = case_batch(c)
    assert not c["opts"] and not any(p[k].any() for k in p if k.endswith("/bias"))
    for scope, ids in (("source_encoder", src), ("target_encoder", tgt)):
        name = scope + "/rnn/basic_lstm_cell/"
        h, tape = O.lstm_forward(p["word_embedding"], p[name + "kernel"], p[name + "bias"], ids, keep_tape=True)
        cmax = max(float(np.abs(np.arctanh(rec[6].astype(np.float64))).max()) for rec in tape)
        assert 1e-5 < cmax < 1e-2, (scope, cmax)
    want, _ = reference_grads(p, params, src, tgt, z)
    assert all(np.abs(g).max() > 0 for g in want.values())


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


# ---- text-CNN ----------------------------------------------------------------------------------------------------------

def _cnn_grads(defect):
    """oracle._cnn_gradients restated, with one defect switched in."""
    def gradients(params, cfg, src_ids, tgt_rows, labels, bf16=False):
        F32 = O.F32
        emb = params["word_embedding"]
        E = emb.shape[1]
        labels = np.asarray(labels, F32)
        ids = O.check_ids(src_ids, emb.shape[0])
        table = params["target_embedding/tgt_seq_embedding"]
        rows = O.check_ids(np.asarray(tgt_rows).reshape(-1), table.shape[0])
        B, T = ids.shape
        pool, tape = O.cnn_forward(params, ids, keep_tape=True, bf16=bf16)
        M = params["source_only_cnn/src_M"]
        raw_s, raw_t = (pool @ M).astype(F32), table[rows]
        ns, nt = O.l2_normalize(raw_s), O.l2_normalize(raw_t)
        loss, acc, cos = O.loss_and_acc(ns, nt, labels)
        dcos = (O.LOGIT_SCALE * (O.sigmoid(O.LOGIT_SCALE * cos) - labels) / F32(B)).astype(F32)[:, None]
        d_s = O._l2_normalize_bwd(raw_s, ns, dcos * nt)
        d_t = O._l2_normalize_bwd(raw_t, nt, dcos * ns)
        grads = {"source_only_cnn/src_M": (pool.T @ d_s).astype(F32),
                 "target_embedding/tgt_seq_embedding": (rows, d_t.astype(F32))}
        dpool = (d_s @ M.T).astype(F32)
        dX = np.zeros((B, T, E), F32)
        x_raw = emb[ids]
        off = 0
        for (fs, nf), (win, hconv) in zip(zip(O.CNN_FILTER_SIZES, O.CNN_NUM_FILTERS), tape):
            W = params["source_only_cnn/conv-maxpool-%d/W" % fs]
            W2 = O.bf16_round(W).reshape(-1, nf) if bf16 and defect != "bf16_dx_unrounded_filters" else W.reshape(-1, nf)
            P = hconv.shape[1]
            if defect == "argmax_last":
                pstar = P - 1 - hconv[:, ::-1, :].argmax(axis=1)
                gradients.moved += int((pstar != hconv.argmax(axis=1)).sum())
            else:
                pstar = hconv.argmax(axis=1)
            g = dpool[:, off:off + nf] * (np.take_along_axis(hconv, pstar[:, None, :], 1)[:, 0, :] > 0)
            if defect == "bf16_dw_unrounded_windows":
                win = np.stack([x_raw[:, p:p + fs, :].reshape(B, -1) for p in range(P)], axis=1)
            sel = win[np.arange(B)[:, None], pstar]
            gw = g.copy()
            if defect == "dw_db_without_last_sequence":
                gw[B - 1] = 0
            if defect == "dw_db_without_last_sequence_of_a_chunk":       # chunks as cnn_dw_kernel cuts them
                per = -(-B // min(-(-B // 32), 128))
                gw[per - 1::per] = 0
            grads["source_only_cnn/conv-maxpool-%d/W" % fs] = np.einsum("bf,bfk->kf", gw, sel).astype(F32).reshape(W.shape)
            gb = dpool[:, off:off + nf] if defect == "db_without_relu_mask" else gw
            grads["source_only_cnn/conv-maxpool-%d/b" % fs] = gb.sum(axis=0).astype(F32)
            gx = O.bf16_round(g) if defect == "dx_g_single_bf16" else g
            dwin = np.einsum("bf,kf->bfk", gx, W2).reshape(B, nf, fs, E)
            for j in range(fs):
                if defect == "dx_without_last_tap_of_width_5" and fs == 5 and j == fs - 1:
                    continue
                np.add.at(dX, (np.arange(B)[:, None], pstar + j), dwin[:, :, j, :])
            off += nf
        grads["word_embedding"] = (ids.reshape(-1), dX.reshape(-1, E))
        return loss, acc, grads
    gradients.moved = 0
    return gradients


@pytest.mark.parametrize("cid", ["cnn", "cnn-bf16", "cnn-dead"])
def test_cnn_restatement_without_defect_is_the_oracle(monkeypatch, cid):
    params, p, src, tgt, z, rows_global, bf16 = _inputs(_case(cid))
    want, want_tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16, float64=False)
    monkeypatch.setattr(O, "_cnn_gradients", _cnn_grads(None))
    got, tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16, float64=False)
    assert np.array_equal(tail, want_tail)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("defect,cid,bars,hits", [
    ("dx_without_last_tap_of_width_5", "cnn-t5", GRAD_BARS_EXACT, ["word_embedding"]),
    ("dx_without_last_tap_of_width_5", "cnn-t80-e50", GRAD_BARS_EXACT, ["word_embedding"]),
    ("dw_db_without_last_sequence", "cnn-chunks", GRAD_BARS_EXACT, ["conv-maxpool-2/W", "conv-maxpool-5/W", "conv-maxpool-3/b"]),
    ("dw_db_without_last_sequence_of_a_chunk", "cnn-chunks", GRAD_BARS_EXACT, ["conv-maxpool-2/W", "conv-maxpool-5/W", "conv-maxpool-3/b"]),
    ("dw_db_without_last_sequence_of_a_chunk", "cnn-b4100", None, ["conv-maxpool-2/W", "conv-maxpool-5/W", "conv-maxpool-3/b"]),
    ("db_without_relu_mask", "cnn-dead", GRAD_BARS_EXACT, ["conv-maxpool-2/b", "conv-maxpool-5/b"]),
    ("bf16_dx_unrounded_filters", "cnn-bf16-12", GRAD_BARS_EXACT, ["word_embedding"]),
    ("bf16_dw_unrounded_windows", "cnn-bf16-12", GRAD_BARS_EXACT, ["conv-maxpool-2/W", "conv-maxpool-5/W"]),
    ("dx_g_single_bf16", "cnn-bf16-12", GRAD_BARS_EXACT, ["word_embedding"]),
    ("dx_g_single_bf16", "cnn-bf16-12", GRAD_BARS_SPLIT, ["word_embedding"]),
    ("dx_g_single_bf16", "cnn-bf16-32", GRAD_BARS_SPLIT, ["word_embedding"]),
])
def test_cnn_backward_defects_are_rejected(monkeypatch, defect, cid, bars, hits):
    """bars None: the bar the case itself runs on.  (At B = 4100 the defect is the last sequence of EVERY chunk: the batch's
    last row alone happens to be a well-classified one whose share of the weight gradients is ~5e-6, below any bar.)  The bf16 defects run the oracle's own bf16 mode on the float32 masters
    (reference_grads rounds the parameters first, which would hide 'unrounded'); without a defect that is the same gradient."""
    c = _case(cid)
    params, p, src, tgt, z, rows_global, bf16 = _inputs(c)
    bars = bars or case_bars(c)
    want, _ = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bf16)

    def run(fn):
        monkeypatch.setattr(O, "_cnn_gradients", lambda pp, cfg, s, t, lab, bf16=False: fn(pp, cfg, s, t, lab, bf16=bf16_mode))
        return reference_grads(p, params, src, tgt, z, rows_global, float64=False)[0]
    bf16_mode = bf16
    check_grads(run(_cnn_grads(None)), want, (bars[0] / 10, bars[1] / 10))      # the same route without the defect passes
    got = run(_cnn_grads(defect))
    with pytest.raises(AssertionError) as e:
        check_grads(got, want, bars)
    for name in hits:
        assert name in str(e.value), (name, str(e.value))


def test_cnn_arg_max_tie_order_does_not_matter_on_these_inputs(monkeypatch):
    """Equal conv values come from bit-equal windows of equal token ids (all-PAD runs, a repeated id), so routing a tie to the
    LAST maximal position gives the same gradients: the weight gradients bit for bit (the same windows), the embedding rows up
    to the order of one float32 sum.  If this ever fails, the case's inputs hold a tie between different windows."""
    c = _case("cnn-hot")
    params, p, src, tgt, z, rows_global, bf16 = _inputs(c)
    want, _ = reference_grads(p, params, src, tgt, z, rows_global, float64=False)
    fn = _cnn_grads("argmax_last")
    monkeypatch.setattr(O, "_cnn_gradients", fn)
    got, _ = reference_grads(p, params, src, tgt, z, rows_global, float64=False)
    assert fn.moved > 100                                    # the switch did move arg-max positions: the check is not vacuous
    for name in want:
        if name == "word_embedding":
            check_grads({name: got[name]}, {name: want[name]}, (1e-6, 1e-6))
        else:
            assert np.array_equal(got[name], want[name]), name
