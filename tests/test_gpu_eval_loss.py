"""Forward-only loss / accuracy / cosines of held-out pairs (sse_eval_loss, sse_eval_loss_rows; csrc/eval_loss.hip) in every
network mode: against the float64 oracle, against the device's own encodings, bit for bit across chunk sizes / pair
de-duplication / the rows form / single rows, against the train step's loss, after weight updates, and for what it must
leave alone (a pending gradient result, variables, slots, step, learning rate).

CASES, the bars and the case construction are shared with the CPU self-test (tests/test_eval_loss_bars.py), which
re-measures the float32 oracle's distance from its float64 run over the same list and checks the margins below.

Bars.  loss: check_tail's rule, LOSS_REL_EXACT * |want| + 1e-7.  acc: 1e-6 absolute.  cos: the project's 25x rule -- the
float32 oracle is 1.6e-7 from its float64 run on a cosine over this case list, 25 x that rounded to one digit is COS_BAR.
The accuracy is a step function of the logit x = 64 cos (it flips where sigmoid(x) = 0.9 or 0.1, |x| = ln 9), so every case
asserts first that no row's |x| is within LN9_MARGIN of ln 9 in the float64 oracle: a cosine error of COS_BAR moves x by
2.6e-4, 40 times less.

Every case names the lstm_path_* counter its evaluation has to move.  Case E (cell size 300) was drafted as the any-shape
case; that holds for the TRAIN step (fused training kernels end at cell size 256), but the evaluation runs the inference
dispatch, whose fused kernels reach cell size 512, so E's 9 rows run the few-sequences kernel and E asserts that counter.
Case G is E with cell size 520, which the inference dispatch does send to the any-shape path (lstm_path_generic)."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import LOSS_REL_EXACT, model_params, oracle_float64, oracle_params, random_ids

pytestmark = pytest.mark.gpu

COS_BAR = 4e-6
ACC_BAR = 1e-6
LN9_MARGIN = 0.01
TABLE = "target_embedding/tgt_seq_embedding"

# id: mode, (V, E, Hs, Ht, S, T), N, B, pad, paired, seed, the lstm_path_* counter an evaluation must move (None: no LSTM).
# A case that silently ran another kernel would prove nothing about the one it names.
CASES = {
    "A": dict(mode="dual-encoder", dims=(500, 50, 96, 64, 50, 12), N=7, B=67, pad=0.5, paired=False, seed=1, path="lstm_path_cluster"),
    "B": dict(mode="shared-encoder", dims=(500, 50, 256, 256, 256, 32), N=7, B=128, pad=0.5, paired=True, seed=1, path="lstm_path_cluster"),
    "C": dict(mode="source-encoder-only", dims=(500, 50, 64, 64, 24, 8), N=7, B=5, pad=0.0, paired=False, seed=0, path="lstm_path_persist"),
    "D": dict(mode="source_only_cnn", dims=(500, 50, 96, 96, 64, 16), N=7, B=37, pad=0.3, paired=False, seed=0, path=None),
    # cell size 300 is outside the fused TRAINING kernels (the train step of this shape runs the any-shape path), but the inference
    # dispatch, which the evaluation goes through, still has a fused kernel for it (cell sizes <= 512): 9 rows -> few-sequences kernel
    "E": dict(mode="dual-encoder", dims=(300, 50, 300, 300, 40, 6), N=7, B=9, pad=0.0, paired=False, seed=0, path="lstm_path_small"),
    "F": dict(mode="dual-encoder", dims=(500, 50, 64, 64, 50, 8), N=7, B=200, pad=0.5, paired=True, seed=0, path="lstm_path_cluster"),
    # E's shape with a cell size the inference dispatch sends to the any-shape path (lstm_generic.hip: cell size > 512)
    "G": dict(mode="dual-encoder", dims=(300, 50, 520, 520, 40, 6), N=7, B=9, pad=0.0, paired=False, seed=0, path="lstm_path_generic"),
}
LSTM_PATHS = ("lstm_path_persist", "lstm_path_cluster", "lstm_path_small", "lstm_path_x3", "lstm_path_generic", "lstm_path_fwd")


def table_mode(cfg):
    return cfg["network_mode"] in ("source-encoder-only", "source_only_cnn")


def build_case(cid):
    """(cfg, oracle parameters, src, tgt, labels) of a case, in the issue's draw order."""
    c = CASES[cid]
    V, E, Hs, Ht, S, T = c["dims"]
    cfg = model_params(c["mode"], V, E, Hs, Ht, S, T, c["N"])
    p = oracle_params(cfg, c["seed"])
    rng = np.random.RandomState(1000 + c["seed"])
    src = random_ids(rng, c["B"], T, V, c["pad"])
    if c["paired"]:
        src[1::2] = src[0::2]
    tgt = rng.randint(0, c["N"], c["B"]).astype(np.int32) if table_mode(cfg) else random_ids(rng, c["B"], T, V, c["pad"])
    if c["paired"]:
        labels = np.tile(np.array([1.0, 0.0], np.float32), c["B"] // 2)
    else:
        labels = rng.randint(0, 2, c["B"]).astype(np.float32)
    return cfg, p, src, tgt, labels


def oracle_eval(p, cfg, src, tgt, labels, float64=True):
    """(loss, acc, cos [B]) from O.encode + O.loss_and_acc, as Python floats / a float64 array."""
    import contextlib
    with (oracle_float64() if float64 else contextlib.nullcontext()):
        q = {k: np.asarray(v, O.F32) for k, v in p.items()}
        ns = O.encode(q, cfg, "src", src, normalize=True)
        nt = O.l2_normalize(q[TABLE][np.asarray(tgt).reshape(-1)]) if table_mode(cfg) else O.encode(q, cfg, "tgt", tgt, normalize=True)
        loss, acc, cos = O.loss_and_acc(ns, nt, np.asarray(labels, O.F32))
    return float(loss), float(acc), np.asarray(cos, np.float64)


def formula_f64(raw_s, raw_t, labels):
    """The loss / acc / cos formula (sse_model.py:282-283,290,298,302) in float64 numpy on given un-normalised rows."""
    s, t, z = np.asarray(raw_s, np.float64), np.asarray(raw_t, np.float64), np.asarray(labels, np.float64)
    cos = (s * t).sum(1) / np.sqrt(np.maximum((s * s).sum(1), 1e-12)) / np.sqrt(np.maximum((t * t).sum(1), 1e-12))
    x = 64.0 * cos
    per = (1.0 - z) * x + np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0)
    sg = 1.0 / (1.0 + np.exp(-x))
    acc = z * np.floor(sg + 0.1) + (1.0 - z) * np.floor(1.1 - sg)
    return float(per.mean()), float(acc.mean()), cos


def ln9_margin(cos):
    return float(np.abs(np.abs(64.0 * np.asarray(cos, np.float64)) - np.log(9.0)).min())


_WANT = {}


def want(cid):
    """The float64 oracle's (loss, acc, cos) of a case: computed once, shared, never modified."""
    if cid not in _WANT:
        cfg, p, src, tgt, labels = build_case(cid)
        loss, acc, cos = oracle_eval(p, cfg, src, tgt, labels)
        cos.setflags(write=False)
        _WANT[cid] = (loss, acc, cos)
    return _WANT[cid]


def model_of(cid, opts=None):
    import sse_amd
    cfg, p, src, tgt, labels = build_case(cid)
    m = sse_amd.SSEModel(cfg)
    m.set_variables(p)
    for k, v in (opts or {}).items():
        m.handle.set_option(k, v)
    return m, cfg, p, src, tgt, labels


def counters(h):
    return {n: h.get_counter(n) for n in LSTM_PATHS + ("eval_paired_calls",)}


def check_against(got, wanted, what):
    """got = (loss, acc, cos) of the device, wanted = the same from a float64 computation with every row clear of ln 9."""
    loss, acc, cos = got
    wl, wa, wc = wanted
    margin = ln9_margin(wc)
    assert margin >= LN9_MARGIN, "%s: a row's |64 cos| is %.4f from ln 9: the accuracy is not decided there" % (what, margin)
    dcos = float(np.abs(np.asarray(cos, np.float64) - wc).max())
    print("\n[eval_loss %s] loss %.9g want %.9g (rel %.2e) | acc %.9g want %.9g | max |d cos| %.2e | ln 9 margin %.3f"
          % (what, loss, wl, abs(float(loss) - wl) / abs(wl), acc, wa, dcos, margin))
    assert cos.dtype == np.float32 and cos.shape == wc.shape
    assert dcos <= COS_BAR, "%s: cos off by %.3g (bar %.0e)" % (what, dcos, COS_BAR)
    assert abs(float(loss) - wl) <= LOSS_REL_EXACT * abs(wl) + 1e-7, "%s: loss %r, want %r" % (what, loss, wl)
    assert abs(float(acc) - wa) <= ACC_BAR, "%s: acc %r, want %r" % (what, acc, wa)


# ---- 1. against the float64 oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(CASES))
def test_matches_the_float64_oracle(cid):
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    before = counters(h)
    loss, acc, cos = h.eval_loss(src, tgt, labels, return_cos=True)
    after = counters(h)
    assert isinstance(loss, np.float32) and isinstance(acc, np.float32)
    check_against((loss, acc, cos), want(cid), cid)
    if cid in ("A", "F"):
        assert 0.0 < want(cid)[1] < 1.0                            # both outcomes of the accuracy occur
    moved = [n for n in LSTM_PATHS if after[n] > before[n]]
    path = CASES[cid]["path"]
    if path is None:
        assert not moved, moved
    else:
        assert path in moved, "%s: expected %s to run, the counters that moved: %s" % (cid, path, moved)
    # without the cosines: the same two numbers
    assert h.eval_loss(src, tgt, labels) == (loss, acc)
    sums = h.eval_loss_sums(src, tgt, labels)
    assert sums[2] == len(labels) and np.float32(sums[0] / sums[2]) == loss and np.float32(sums[1] / sums[2]) == acc


# ---- 2. against the device's own encodings -------------------------------------------------------------------------
@pytest.mark.parametrize("cid,opts", [(c, None) for c in sorted(CASES)] + [("D", dict(cnn_bf16=1)), ("B", dict(lstm_x3=1))],
                         ids=sorted(CASES) + ["D-cnn_bf16", "B-lstm_x3"])
def test_matches_the_formula_on_the_devices_own_encodings(cid, opts):
    import sse_amd
    m, cfg, p, src, tgt, labels = model_of(cid, opts)
    h = m.handle
    raw_s = h.encode(sse_amd._lib.SIDE_SOURCE, src, normalize=False)
    raw_t = p[TABLE][tgt] if table_mode(cfg) else h.encode(sse_amd._lib.SIDE_TARGET, tgt, normalize=False)
    wanted = formula_f64(raw_s, raw_t, labels)
    got = h.eval_loss(src, tgt, labels, return_cos=True)
    what = cid + ("" if not opts else " " + ",".join(opts))
    check_against(got, wanted, what + " (own encodings)")


# ---- 3. bit identities ---------------------------------------------------------------------------------------------
def _bytes(res):
    return (np.float32(res[0]).tobytes(), np.float32(res[1]).tobytes(), res[2].tobytes())


def test_chunk_size_does_not_change_a_bit():
    m, cfg, p, src, tgt, labels = model_of("F")
    h = m.handle
    ref = _bytes(h.eval_loss(src, tgt, labels, return_cos=True))   # default chunk: one chunk
    for rows in (2, 64, 66, 67):                                   # 67 is rounded down to 66
        h.set_option("eval_chunk_rows", rows)
        assert _bytes(h.eval_loss(src, tgt, labels, return_cos=True)) == ref, rows
    with pytest.raises(sse_amd_error()):
        h.set_option("eval_chunk_rows", 1)
    # an unpaired batch in chunks that leave a partial one
    m, cfg, p, src, tgt, labels = model_of("A")
    ref = _bytes(m.handle.eval_loss(src, tgt, labels, return_cos=True))
    m.handle.set_option("eval_chunk_rows", 10)
    assert _bytes(m.handle.eval_loss(src, tgt, labels, return_cos=True)) == ref


def sse_amd_error():
    import sse_amd
    return sse_amd.SSEError


@pytest.mark.parametrize("cid", ["B", "F"])
def test_pair_dedup_does_not_change_a_bit(cid):
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    h.set_option("train_pair_dedup", 0)
    plain = _bytes(h.eval_loss(src, tgt, labels, return_cos=True))
    assert h.get_counter("eval_paired_calls") == 0
    h.set_option("train_pair_dedup", 1)
    assert _bytes(h.eval_loss(src, tgt, labels, return_cos=True)) == plain
    assert h.get_counter("eval_paired_calls") == 1


def test_a_batch_with_one_broken_pair_runs_unpaired_and_matches_the_oracle():
    m, cfg, p, src, tgt, labels = model_of("F")
    src = src.copy()
    src[1, -2] = 2 + (src[1, -2] - 1) % (cfg["vocab_size"] - 2)    # another valid token: rows 0 and 1 differ now
    assert not np.array_equal(src[0], src[1])
    got = m.handle.eval_loss(src, tgt, labels, return_cos=True)
    assert m.handle.get_counter("eval_paired_calls") == 0
    check_against(got, oracle_eval(p, cfg, src, tgt, labels), "F with a broken pair")


@pytest.mark.parametrize("cid", ["A", "C", "F"])
def test_rows_form_equals_ids_form(cid):
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    rng = np.random.RandomState(5)
    B = len(labels)
    h.corpus_upload(0, src)
    src_rows = rng.randint(0, B, B).astype(np.int32)
    if CASES[cid]["paired"]:
        src_rows[1::2] = src_rows[0::2]
    if table_mode(cfg):
        tgt_rows, tgt_ids = tgt, tgt
    else:
        h.corpus_upload(1, tgt)
        tgt_rows = rng.randint(0, B, B).astype(np.int32)
        tgt_ids = tgt[tgt_rows]
    by_ids = h.eval_loss(src[src_rows], tgt_ids, labels, return_cos=True)
    by_rows = h.eval_loss_rows(src_rows, tgt_rows, labels, return_cos=True)
    assert _bytes(by_rows) == _bytes(by_ids)
    assert h.eval_loss_rows(src_rows, tgt_rows, labels) == by_ids[:2]
    assert h.eval_loss_rows_sums(src_rows, tgt_rows, labels) == h.eval_loss_sums(src[src_rows], tgt_ids, labels)
    if CASES[cid]["paired"]:
        assert h.get_counter("eval_paired_calls") == 5              # every call above


@pytest.mark.parametrize("cid", sorted(CASES))
def test_every_row_alone_has_the_same_cosine(cid):
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    _, _, cos = h.eval_loss(src, tgt, labels, return_cos=True)
    alone = np.array([h.eval_loss(src[b:b + 1], tgt[b:b + 1], labels[b:b + 1], return_cos=True)[2][0] for b in range(len(labels))])
    assert alone.tobytes() == cos.tobytes(), np.flatnonzero(alone != cos)


@pytest.mark.parametrize("cid", ["A", "C"])
def test_a_cluster_kernel_give_up_re_runs_the_call_on_the_other_kernels(cid):
    """The cluster kernels report a workgroup that did not arrive through the error flag (testing aid
    lstm_persist_inject_miss raises it after every cluster launch): the evaluation runs once more on the kernels that need
    no co-residency, which are bit-identical, and counts a fall-back like the host-buffer encodes do."""
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    ref = _bytes(h.eval_loss(src, tgt, labels, return_cos=True))
    h.set_option("lstm_persist_inject_miss", 1)
    before = h.get_counter("lstm_persist_fallbacks"), h.get_counter("lstm_path_small")
    assert _bytes(h.eval_loss(src, tgt, labels, return_cos=True)) == ref
    assert h.get_counter("lstm_persist_fallbacks") == before[0] + 1 and h.get_counter("lstm_path_small") > before[1]
    h.set_option("lstm_persist_inject_miss", 0)
    assert _bytes(h.eval_loss(src, tgt, labels, return_cos=True)) == ref      # (backed off or not: the same bits)


# ---- 4. the same loss as the train step ----------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["A", "B", "C", "D"])
def test_same_loss_as_the_train_step_of_the_same_batch(cid):
    m, cfg, p, src, tgt, labels = model_of(cid)
    wl, wa, wc = want(cid)
    assert ln9_margin(wc) >= LN9_MARGIN
    loss, acc = m.handle.eval_loss(src, tgt, labels)
    t_loss, t_acc = m.handle.train_step(src, tgt, labels)          # evaluated before its update
    print("\n[eval_loss %s] eval %.9g train step %.9g oracle %.9g" % (cid, loss, t_loss, wl))
    assert abs(float(loss) - wl) <= LOSS_REL_EXACT * abs(wl) and abs(t_loss - wl) <= LOSS_REL_EXACT * abs(wl)
    assert abs(float(loss) - t_loss) <= 2 * LOSS_REL_EXACT * abs(wl)
    assert abs(float(acc) - t_acc) <= ACC_BAR


# ---- 5. no stale weights -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["A", "D"])
def test_evaluates_the_weights_two_train_steps_left(cid):
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    h.eval_loss(src, tgt, labels)                                   # (layouts packed from the initial weights)
    for _ in range(2):
        h.train_step(src, tgt, labels)
    now = m.get_variables()
    assert any(not np.array_equal(now[k], p[k]) for k in p)
    got = h.eval_loss(src, tgt, labels, return_cos=True)
    check_against(got, oracle_eval(now, cfg, src, tgt, labels), cid + " after two steps")


# ---- 6. nothing else changes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["A", "D", "F"])
def test_a_pending_gradient_result_survives_an_evaluation(cid):
    import torch
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    arena = torch.full((h.train_grad_count(),), float("nan"), dtype=torch.float32, device="cuda:0")
    h.train_bind_arena(arena)
    h.train_grads(src, tgt, labels)
    torch.cuda.synchronize()
    kept = arena.clone()
    other_src = np.roll(src, 1, axis=0)                            # another batch than the pending one
    h.eval_loss(other_src, tgt, labels, return_cos=True)
    torch.cuda.synchronize()
    assert arena.cpu().numpy().tobytes() == kept.cpu().numpy().tobytes()
    loss, acc = h.train_apply()
    tail = kept[-4:].cpu().numpy()
    assert np.float32(loss) == tail[1] and np.float32(acc) == tail[2] and h.global_step == 1


@pytest.mark.parametrize("cid", ["B", "C"])
def test_variables_slots_step_and_learning_rate_are_unchanged(cid):
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    h.train_step(src, tgt, labels)                                  # slots away from their initial value
    h.decay_learning_rate()
    before = {k: v.tobytes() for k, v in m.get_variables(with_slots=True).items()}
    step, lr = h.global_step, h.learning_rate
    h.eval_loss(src, tgt, labels, return_cos=True)
    after = {k: v.tobytes() for k, v in m.get_variables(with_slots=True).items()}
    assert after == before and h.global_step == step == 1 and h.learning_rate == lr


def test_data_parallel_trainer_on_one_rank_is_the_handles_evaluation():
    import sse_amd
    m, cfg, p, src, tgt, labels = model_of("A")
    h = m.handle
    tr = sse_amd.DataParallelTrainer(h, device="cuda:0")
    loss, acc = h.eval_loss(src, tgt, labels)
    got = tr.eval_loss(src, tgt, labels)
    assert (np.float32(got[0]), np.float32(got[1])) == (loss, acc)
    h.corpus_upload(0, src)
    h.corpus_upload(1, tgt)
    rows = np.arange(len(labels), dtype=np.int32)
    assert tr.eval_loss(rows, rows, labels, by_rows=True) == got
    assert tr.train_step(src, tgt, labels)[0] == pytest.approx(float(loss), rel=2 * LOSS_REL_EXACT)   # the trainer still trains


# ---- 7. errors -----------------------------------------------------------------------------------------------------
def test_ids_and_rows_out_of_range_are_errors_and_the_next_call_is_clean():
    import sse_amd
    m, cfg, p, src, tgt, labels = model_of("A")
    h = m.handle
    good = _bytes(h.eval_loss(src, tgt, labels, return_cos=True))
    for side in (0, 1):
        bad = [src.copy(), tgt.copy()]
        bad[side][3, -2] = cfg["vocab_size"]
        with pytest.raises(sse_amd.SSEError, match="out of range"):
            h.eval_loss(bad[0], bad[1], labels, return_cos=True)
        assert _bytes(h.eval_loss(src, tgt, labels, return_cos=True)) == good
    h.corpus_upload(0, src)
    h.corpus_upload(1, tgt)
    rows = np.arange(len(labels), dtype=np.int32)
    assert _bytes(h.eval_loss_rows(rows, rows, labels, return_cos=True)) == good
    for side in (0, 1):
        bad = [rows.copy(), rows.copy()]
        bad[side][7] = len(labels)
        with pytest.raises(sse_amd.SSEError, match="out of range"):
            h.eval_loss_rows(bad[0], bad[1], labels)
        assert _bytes(h.eval_loss_rows(rows, rows, labels, return_cos=True)) == good
    assert h.eval_loss_sums(src[:0], tgt[:0], labels[:0]) == (0.0, 0.0, 0.0)
    assert h.eval_loss_rows_sums(rows[:0], rows[:0], labels[:0]) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("cid", ["C", "D"])
def test_a_target_matrix_row_out_of_range_is_an_error(cid):
    import sse_amd
    m, cfg, p, src, tgt, labels = model_of(cid)
    h = m.handle
    good = _bytes(h.eval_loss(src, tgt, labels, return_cos=True))
    for bad_row in (CASES[cid]["N"], -1):
        bad = tgt.copy()
        bad[2] = bad_row
        with pytest.raises(sse_amd.SSEError, match="out of range"):
            h.eval_loss(src, bad, labels, return_cos=True)
        assert _bytes(h.eval_loss(src, tgt, labels, return_cos=True)) == good
    with pytest.raises(ValueError):                                 # token ids where this mode wants target rows
        h.eval_loss(src, src, labels)


def test_rows_form_without_a_corpus_is_an_error():
    import sse_amd
    m, cfg, p, src, tgt, labels = model_of("A")
    rows = np.arange(len(labels), dtype=np.int32)
    with pytest.raises(sse_amd.SSEError, match="corpus"):
        m.handle.eval_loss_rows(rows, rows, labels)
    m.handle.corpus_upload(0, src)
    with pytest.raises(sse_amd.SSEError, match="corpus"):
        m.handle.eval_loss_rows(rows, rows, labels)


# ---- 8. Session.run ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["A", "D"])
def test_session_run_fetches_without_train_run_one_evaluation(cid):
    import sse_amd
    m, cfg, p, src, tgt, labels = model_of(cid)
    sess = sse_amd.Session(m)
    feed = m.get_train_feed_dict(src, tgt, labels)
    loss, acc, cos = m.eval_loss(src, tgt, labels, return_cos=True)
    path = CASES[cid]["path"]
    per_eval = 2 if cid == "A" else 0                               # encodes of one evaluation (dual-encoder: two)

    def run(fetches):
        before = m.handle.get_counter(path) if path else 0
        out = sess.run(fetches, feed)
        if path:
            assert m.handle.get_counter(path) - before == per_eval
        return out

    assert tuple(run([m.loss, m.train_acc])) == (loss, acc)
    assert run(m.loss) == loss
    got = run([m.binarylogit])
    assert len(got) == 1 and got[0].tobytes() == cos.tobytes()
    l2, c2, a2 = run([m.loss, m.binarylogit, m.train_acc])
    assert (l2, a2) == (loss, acc) and c2.tobytes() == cos.tobytes()
    assert m.handle.global_step == 0
    with pytest.raises(KeyError):
        sess.run([m.train, m.binarylogit], feed)
    assert m.handle.global_step in (0, 1)
    step = m.handle.global_step
    _, t_loss, t_acc = sess.run([m.train, m.loss, m.train_acc], feed)   # as before: one train step, its loss
    assert m.handle.global_step == step + 1 and isinstance(t_loss, float)
