"""The train step under option train_class_loss = 1 (softmax over the whole free target matrix): sse_train_grads into a
NaN-filled arena against the float64 step of tests/class_loss_cases.py on every variable and the tail, on the fused, any-shape
and text-CNN paths, by ids and by corpus rows; sse_train_step against sse_train_grads + sse_train_apply and a float64 clip +
Adagrad with the table dense; the refusals; a state walk on one handle against fresh handles; one short learning run against a
free-running float64 reference."""
import numpy as np
import pytest

from tests import class_loss_cases as CC
from tests import inbatch_cases as IC
from tests.util import arena_grads

pytestmark = pytest.mark.gpu

PATH_COUNTER = {"fused": "train_path_fused", "generic": "train_path_generic", "cnn": "train_path_cnn"}
TRAIN_COUNTERS = ("train_path_fused", "train_path_generic", "train_path_cnn", "train_paired_steps", "train_inbatch_steps",
                  "train_class_steps")
EMB = "word_embedding"        # its gradient is scattered with float atomics (tests/test_gpu_train_state.py); a class step's table is not


def _model(c, p, params, class_loss=True):
    import sse_amd
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    for k, v in c["opts"].items():
        m.handle.set_option(k, v)
    if class_loss:
        m.handle.set_option("train_class_loss", 1)
        m.handle.set_option("train_loss_scale", c["scale"])
    return m


def _corpus_rows(m, src):
    """The sources as a shuffled device corpus; returns the corpus row of every batch row."""
    order = np.random.RandomState(5).permutation(len(src)).astype(np.int32)
    m.handle.corpus_upload(0, src[order])
    return np.argsort(order).astype(np.int32)


def _arena(c, m, src, tgt, z, rows_global=None):
    if not c["by_rows"]:
        return arena_grads(m, src, tgt, z, rows_global)
    return arena_grads(m, _corpus_rows(m, src), tgt, z, rows_global, rows=True)


@pytest.mark.parametrize("c", CC.STEP_CASES, ids=[c["id"] for c in CC.STEP_CASES])
def test_class_step_gradients_match_float64(c):
    params, p, src, tgt, z, want, want_tail, _ = CC.step_case_seeded(c)
    m = _model(c, p, params)
    h = m.handle
    got, tail = _arena(c, m, src, tgt, z)
    for path, counter in PATH_COUNTER.items():
        assert h.get_counter(counter) == (1 if path == c["path"] else 0), counter
    assert h.get_counter("train_class_steps") == 1 and h.get_counter("train_inbatch_steps") == 0
    for n, g in got.items():
        assert not np.isnan(g).any(), "%s: an element of %s was not written" % (c["id"], n)
    errs = CC.check_step(got, tail, want, want_tail, c)
    unnamed = ~np.isin(np.arange(c["N"]), tgt)
    assert unnamed.any() and np.abs(got[CC.TABLE][unnamed]).max() > 0       # dense: also on classes no row names
    print("CLASS GRADERR %s bars %.1e/%.1e: norm %.2e element %.2e; loss %r want %r"
          % (c["id"], c["bars"][0], c["bars"][1], max(e[0] for e in errs.values()), max(e[1] for e in errs.values()),
             float(tail[1]), float(want_tail[1])))


def _bits_equal(a, b, what, skip=(EMB,)):
    for n in a:
        if n.split("/Adagrad")[0] in skip:
            continue
        assert np.array_equal(np.asarray(a[n]).view(np.uint32), np.asarray(b[n]).view(np.uint32)), "%s: %s" % (what, n)


@pytest.mark.parametrize("cid,table_scale", [("seo-fused-b70-n40", 1.0), ("seo-fused-b70-n40", 0.01), ("cnn-b6-n571", 1.0)],
                         ids=["seo", "seo-clip-engaged", "cnn"])
def test_step_equals_grads_plus_apply_and_a_float64_clip_and_adagrad_with_the_table_dense(cid, table_scale):
    """table_scale 0.01: the table's rows 100 times shorter, its gradient 100 times larger -- the global norm passes 5 and the
    clip engages, with the table's whole gradient in the norm."""
    c = dict(CC.STEP_CASES_BY_ID[cid], by_rows=False)
    params, p, src, tgt, z = CC.step_case_seeded(CC.STEP_CASES_BY_ID[cid])[:5]
    p = dict(p)
    p[CC.TABLE] = (p[CC.TABLE] * np.float32(table_scale)).astype(np.float32)
    one, two = _model(c, p, params), _model(c, p, params)
    h = two.handle
    got, tail = arena_grads(two, src, tgt, z)
    before = two.get_variables(with_slots=True)
    names = [n for n, _, _, _ in h.variables()]
    wv, ws, clip = CC.reference_apply(got, tail, {n: before[n] for n in names}, {n: before[n + "/Adagrad"] for n in names}, h.learning_rate)
    if table_scale != 1.0:
        assert clip < 1.0, clip
    loss, acc = h.train_apply()
    assert (loss, acc) == (float(tail[1]), float(tail[2]))
    after = two.get_variables(with_slots=True)
    for n in names:
        for have, ref, what in ((after[n], wv[n], n), (after[n + "/Adagrad"], ws[n], n + "/Adagrad")):
            d = np.abs(have.astype(np.float64) - ref.reshape(have.shape)) / np.maximum(1.0, np.abs(ref.reshape(have.shape)))
            assert d.max() <= 1e-6, (what, float(d.max()))
    unnamed = ~np.isin(np.arange(c["N"]), tgt)
    assert (np.abs(after[CC.TABLE] - before[CC.TABLE]).max(axis=1) > 0)[unnamed].any()   # classes no row names moved too
    # the fused entry point: the same loss, the same variables
    loss1, acc1 = one.train_step(src, tgt, z)
    assert (loss1, acc1) == (loss, acc)
    stepped = one.get_variables(with_slots=True)
    _bits_equal(stepped, after, cid)
    assert np.allclose(stepped[EMB], after[EMB], rtol=1e-5, atol=1e-7)
    assert one.handle.get_counter("train_class_steps") == 1 and h.get_counter("train_class_steps") == 1


def test_refusals_leave_the_handle_usable():
    import sse_amd
    for mode in ("dual-encoder", "shared-encoder"):
        c = dict(IC.STEP_CASES_BY_ID["dual-unpaired-b40"], mode=mode)
        params, p = IC.step_params(c)
        src, tgt, z = IC.step_batch(c)
        m, fresh = (_plain_model(p, params) for _ in range(2))
        m.handle.set_option("train_class_loss", 1)
        before = m.get_variables(with_slots=True)
        for call in (lambda: m.train_step(src, tgt, z), lambda: m.handle.train_grads(src, tgt, z, rows_global=len(z))):
            with pytest.raises(sse_amd.SSEError, match="train_class_loss = 1 needs a network mode with a free target matrix"):
                call()
        with pytest.raises(sse_amd.SSEError, match="no gradients pending"):
            m.handle.train_apply()
        for counter in TRAIN_COUNTERS:
            assert m.handle.get_counter(counter) == 0, counter
        _bits_equal(m.get_variables(with_slots=True), before, mode, skip=())
        m.handle.set_option("train_class_loss", 0)
        assert m.train_step(src, tgt, z) == fresh.train_step(src, tgt, z)
        _bits_equal(m.get_variables(with_slots=True), fresh.get_variables(with_slots=True), mode + " pair step after the refusal")
    # two objectives at once
    c = CC.STEP_CASES_BY_ID["seo-fused-b70-n40"]
    params, p, src, tgt, z = CC.step_case_seeded(c)[:5]
    m, fresh = _model(c, p, params), _model(c, p, params, class_loss=False)
    m.handle.set_option("train_loss", 1)
    with pytest.raises(sse_amd.SSEError, match="train_class_loss = 1 and train_loss = 1 ask for two objectives"):
        m.train_step(src, tgt, z)
    for counter in TRAIN_COUNTERS:
        assert m.handle.get_counter(counter) == 0, counter
    m.handle.set_option("train_class_loss", 0)
    m.handle.set_option("train_loss", 0)
    assert m.train_step(src, tgt, z) == fresh.train_step(src, tgt, z)
    _bits_equal(m.get_variables(with_slots=True), fresh.get_variables(with_slots=True), "pair step after the refusal",
                skip=(EMB, CC.TABLE))


def test_a_bad_target_row_cancels_the_step_and_leaves_the_handle_usable():
    """No gather runs in a class step: the head itself finds a target row outside [0, N).  sse_train_step reports it with the
    loss and has cancelled its update on the device; sse_train_grads reports it at once and leaves no gradients pending."""
    import sse_amd
    c = CC.STEP_CASES_BY_ID["seo-fused-b70-n40"]
    params, p, src, tgt, z = CC.step_case_seeded(c)[:5]
    m, fresh = _model(c, p, params), _model(c, p, params)
    for row, value in ((3, c["N"]), (0, -1)):
        bad = tgt.copy()
        bad[row] = value
        before = m.get_variables(with_slots=True)
        with pytest.raises(sse_amd.SSEError, match="out of range"):
            m.train_step(src, bad, z)
        _bits_equal(m.get_variables(with_slots=True), before, "cancelled update", skip=())
        with pytest.raises(sse_amd.SSEError, match="out of range"):
            m.handle.train_grads(src, bad, z, rows_global=len(z))
        with pytest.raises(sse_amd.SSEError, match="no gradients pending"):
            m.handle.train_apply()
    assert m.train_step(src, tgt, z) == fresh.train_step(src, tgt, z)
    _bits_equal(m.get_variables(with_slots=True), fresh.get_variables(with_slots=True), "class step after the bad rows")


def _plain_model(p, params):
    import sse_amd
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    return m


def _set_objective(h, kind):
    h.set_option("train_class_loss", 1 if kind == "class" else 0)
    h.set_option("train_loss", 1 if kind == "inbatch" else 0)


def test_state_walk_on_one_handle_equals_fresh_handles():
    """class step, pair step, in-batch step, class step, then sse_train_grads of a class batch with the option switched off
    before sse_train_apply -- every call on the long-lived handle and on a fresh handle given its variables and slots.  Bit for
    bit on every variable whose gradient is reduced in a fixed order (all but word_embedding, and the table under the pair and
    in-batch losses, which scatter with float atomics), the loss, the accuracy and the train_* counters' increments.  A
    dense-table mark left behind by the class step would put the table's scattered gradient into the global norm twice over
    in the pair step (tail[0] and whole); one not remembered across the toggle would drop it from the last apply."""
    c = CC.STEP_CASES_BY_ID["seo-fused-b70-n40"]
    params, p = CC.step_params(c)
    p = dict(p)
    p[CC.TABLE] = (p[CC.TABLE] * np.float32(0.01)).astype(np.float32)      # the clip engages: the global norm shows in every variable
    lr = 1e-3                                   # the table stays short over the walk: the clip engages at every step
    long_lived = _model(c, p, params, class_loss=False)
    long_lived.handle.learning_rate = lr
    walk = [("class", 70), ("pair", 70), ("inbatch", 38), ("class", 70), ("class-toggled", 38)]
    before = long_lived.get_variables(with_slots=True)
    for step, (kind, B) in enumerate(walk):
        src, tgt, z = CC.step_batch(c, seed=10 + step, B=B)
        fresh = _model(c, p, params, class_loss=False)
        fresh.set_variables(long_lived.get_variables(with_slots=True))
        fresh.handle.learning_rate = lr
        results = []
        for m in (long_lived, fresh):
            h = m.handle
            c0 = {n: h.get_counter(n) for n in TRAIN_COUNTERS}
            if kind == "class-toggled":
                _set_objective(h, "class")
                h.train_grads(src, tgt, z, rows_global=len(z))
                _set_objective(h, "pair")
                out = h.train_apply()
            else:
                _set_objective(h, kind)
                out = m.train_step(src, tgt, z)
            results.append((out, m.get_variables(with_slots=True), {n: h.get_counter(n) - c0[n] for n in TRAIN_COUNTERS}))
        (o1, v1, d1), (o2, v2, d2) = results
        what = "step %d (%s, B %d)" % (step, kind, B)
        assert o1 == o2, (what, o1, o2)
        assert d1 == d2, (what, d1, d2)
        assert d1["train_class_steps"] == (1 if kind.startswith("class") else 0) and d1["train_inbatch_steps"] == (1 if kind == "inbatch" else 0)
        _bits_equal(v1, v2, what, skip=(EMB,) if kind.startswith("class") else (EMB, CC.TABLE))
        for n in (EMB, CC.TABLE):
            assert np.allclose(v1[n], v2[n], rtol=1e-5, atol=1e-7), (what, n)
        if kind == "class-toggled":   # the apply took the table whole: float64 clip + Adagrad of a fresh handle's own arena
            ref = _model(c, p, params)
            ref.set_variables(before)
            ref.handle.learning_rate = lr
            got, tail = arena_grads(ref, src, tgt, z)
            names = [n for n, _, _, _ in ref.handle.variables()]
            wv, _, clip = CC.reference_apply(got, tail, {n: before[n] for n in names}, {n: before[n + "/Adagrad"] for n in names},
                                             ref.handle.learning_rate)
            assert clip < 1.0
            for n in names:
                d = np.abs(v1[n].astype(np.float64) - wv[n].reshape(v1[n].shape)) / np.maximum(1.0, np.abs(wv[n].reshape(v1[n].shape)))
                assert d.max() <= 1e-6, (n, float(d.max()))
        before = long_lived.get_variables(with_slots=True)


@pytest.mark.parametrize("cid", ["seo-fused-b70-n40", "seo-generic-b70-n40", "cnn-b6-n571"])
def test_class_loss_0_is_the_default_step_bit_for_bit(cid):
    c = dict(CC.STEP_CASES_BY_ID[cid], by_rows=False)
    params, p, src, tgt, z = CC.step_case_seeded(CC.STEP_CASES_BY_ID[cid])[:5]
    explicit, default = _model(c, p, params, class_loss=False), _model(c, p, params, class_loss=False)
    explicit.handle.set_option("train_class_loss", 1)           # there and back again
    explicit.handle.set_option("train_class_loss", 0)
    a, b = arena_grads(explicit, src, tgt, z), arena_grads(default, src, tgt, z)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    _bits_equal(a[0], b[0], cid, skip=(EMB, CC.TABLE))
    for h in (explicit.handle, default.handle):
        assert {n: h.get_counter(n) for n in TRAIN_COUNTERS} == dict({n: 0 for n in TRAIN_COUNTERS}, **{PATH_COUNTER[c["path"]]: 1})


def test_class_loss_falls_and_tracks_a_free_running_float64_reference():
    """The learning run of tests/class_loss_cases.py (60 steps, 32 pair rows, 40 classes, lr 0.003): the device against float64
    gradients + float64 clip and Adagrad, table dense, run freely from the same initial weights.  Asserted: the loss of every
    step within learn_loss_bar of the free-running curve, every element of every final variable within learn_variable_bar
    of the reference's (a drift in the dense-table norm or Adagrad over the steps shows there), and the loss ends below where
    it began.  The run is shaped so that these bars can hold; tests/test_class_loss_cases_host.py holds the float32
    restatement to them and shows what lr 0.05 does to it."""
    params, p, src, tgt, z = CC.learn_setup()
    m = _model(dict(opts={}, scale=CC.LEARN_SCALE), p, params)
    h = m.handle
    h.learning_rate = CC.LEARN_LR
    start = m.get_variables(with_slots=True)
    for n, _, _, _ in h.variables():
        assert np.array_equal(start[n + "/Adagrad"].reshape(-1), np.full(start[n].size, 0.1, np.float32)), n
    ref = CC.learn_free_run()
    got = [m.train_step(src, tgt, z)[0] for _ in range(CC.LEARN_STEPS)]
    loss_share, var_share = CC.check_learning_run(got, m.get_variables(), ref, z)
    print("CLASS LEARN loss %.4f -> %.4f (free-running float64 %.4f -> %.4f); worst |diff| / bar: loss %.2g, final variables %.2g"
          % (got[0], got[-1], ref["loss"][0], ref["loss"][-1], loss_share, var_share))
    assert h.get_counter("train_class_steps") == CC.LEARN_STEPS
