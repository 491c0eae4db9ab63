"""The train step under option train_loss = 1 (in-batch softmax): sse_train_grads into a NaN-filled arena against the float64
step of tests/inbatch_cases.py on every variable and the tail, sse_train_apply against a float64 clip + Adagrad of the
device's own arena, the route of every case proven by counters; a state walk on one handle compared bit for bit with fresh
handles; train_loss = 0 bit-identical to a default handle; one short learning run against a free-running float64 reference."""
import numpy as np
import pytest

from tests import inbatch_cases as IC
from tests.test_gpu_train_state import ATOMIC
from tests.util import arena_grads, reference_apply, split_arena

pytestmark = pytest.mark.gpu

PATH_COUNTER = {"fused": "train_path_fused", "generic": "train_path_generic", "cnn": "train_path_cnn"}


def _model(c, p, params, inbatch=True):
    import sse_amd
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    for k, v in c["opts"].items():
        m.handle.set_option(k, v)
    if inbatch:
        m.handle.set_option("train_loss", 1)
        m.handle.set_option("train_loss_scale", c["scale"])
    return m


def _arena(c, m, src, tgt, z, rows_global):
    """sse_train_grads, or -- by_rows -- sse_train_grads_rows on uploaded, shuffled corpora: rows of equal tokens are different
    corpus rows there."""
    if not c["by_rows"]:
        return arena_grads(m, src, tgt, z, rows_global)
    B = len(z)
    order = np.random.RandomState(5).permutation(B).astype(np.int32)
    inv = np.argsort(order).astype(np.int32)
    m.handle.corpus_upload(0, src[order])
    m.handle.corpus_upload(1, tgt[order])
    assert len(np.unique(src, axis=0)) < B and len(np.unique(tgt, axis=0)) < B      # equal tokens under different row numbers
    return arena_grads(m, inv, inv, z, rows_global, rows=True)


@pytest.mark.parametrize("c", IC.STEP_CASES, ids=[c["id"] for c in IC.STEP_CASES])
def test_inbatch_step_gradients_and_apply_match_float64(c):
    params, p, src, tgt, z, want, want_tail, _ = IC.step_case_seeded(c)
    m = _model(c, p, params)
    h = m.handle
    rows_global = c["rows_factor"] * len(z)
    got, tail = _arena(c, m, src, tgt, z, rows_global)
    # the route
    for path, counter in PATH_COUNTER.items():
        assert h.get_counter(counter) == (1 if path == c["path"] else 0), counter
    assert h.get_counter("train_inbatch_steps") == 1
    assert h.get_counter("train_paired_steps") == (1 if c["paired"] else 0)
    errs = IC.check_step(got, tail, want, want_tail, c)
    # sse_train_apply on its own: float64 clip + Adagrad of the device's own arena
    before = m.get_variables(with_slots=True)
    names = [n for n, _, _, _ in h.variables()]
    wv, ws = reference_apply(got, tail, {n: before[n] for n in names}, {n: before[n + "/Adagrad"] for n in names}, h.learning_rate)
    loss, acc = h.train_apply()
    assert (loss, acc) == (float(tail[1]), float(tail[2]))
    after = m.get_variables(with_slots=True)
    for n in names:
        for have, ref, what in ((after[n], wv[n], n), (after[n + "/Adagrad"], ws[n], n + "/Adagrad")):
            d = np.abs(have.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
            assert d.max() <= 1e-6, (what, float(d.max()))
    print("INBATCH GRADERR %s bars %.1e/%.1e: norm %.2e element %.2e; loss %r want %r"
          % (c["id"], c["bars"][0], c["bars"][1], max(e[0] for e in errs.values()), max(e[1] for e in errs.values()),
             float(tail[1]), float(want_tail[1])))


def _same_bits(a, b, what):
    """Two (blocks, tail) arenas: the same bits in the whole tail and in every variable whose gradient is reduced in a fixed
    order, i.e. all but the two lookup tables, which the backward kernels scatter with float atomics (tests/test_gpu_train_state.py);
    a difference in d(raw encodings) reaches every dense variable."""
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "%s: tail %r / %r" % (what, a[1], b[1])
    for n in a[0]:
        assert not np.isnan(a[0][n]).any(), (what, n)
        if n not in ATOMIC:
            assert np.array_equal(a[0][n].view(np.uint32), b[0][n].view(np.uint32)), "%s: %s" % (what, n)


def _walk_case(B):
    return dict(IC.STEP_CASES_BY_ID["dual-unpaired-b40"], B=B, id="walk-b%d" % B)


def test_state_walk_on_one_handle_equals_fresh_handles_bit_for_bit():
    """B 96 -> 40 -> 96, train_loss 1 -> 0 -> 1, train_loss_scale 64 -> 20 -> 64 on one handle; every call against a fresh
    handle with the same weights and options: stale keys, stale rows B .. Bp of a grown buffer or a scale left behind show."""
    import torch
    walk = [(96, 1, 64), (40, 1, 64), (96, 1, 64), (96, 0, 64), (96, 1, 64), (96, 1, 20), (40, 1, 20), (96, 1, 64)]
    c0 = _walk_case(96)
    params, p = IC.step_params(c0)
    long_lived = _model(c0, p, params)
    for step, (B, loss, scale) in enumerate(walk):
        c = _walk_case(B)
        src, tgt, z = IC.step_batch(c, seed=step)
        fresh = _model(c, p, params)
        arenas = []
        for m in (long_lived, fresh):
            m.handle.set_option("train_loss", loss)
            m.handle.set_option("train_loss_scale", scale)
            h = m.handle
            arena = torch.full((h.train_grad_count(),), float("nan"), dtype=torch.float32, device="cuda:0")
            h.train_bind_arena(arena)
            h.train_grads(src, tgt, z, rows_global=len(z))
            torch.cuda.synchronize()
            arenas.append(split_arena(m, arena.cpu().numpy()))
        _same_bits(arenas[0], arenas[1], "step %d (B %d, train_loss %d, scale %d)" % (step, B, loss, scale))
    assert long_lived.handle.get_counter("train_inbatch_steps") == sum(1 for _, loss, _ in walk if loss == 1)


@pytest.mark.parametrize("cid", ["dual-paired-b128", "seo-b40", "generic-forced", "cnn-b10"])
def test_train_loss_0_is_the_default_step_bit_for_bit(cid):
    c = IC.STEP_CASES_BY_ID[cid]
    params, p = IC.step_params(c)
    src, tgt, z = IC.step_batch(c)
    explicit, default = _model(c, p, params, inbatch=False), _model(c, p, params, inbatch=False)
    explicit.handle.set_option("train_loss", 1)           # there and back again
    explicit.handle.set_option("train_loss_scale", 20)
    explicit.handle.set_option("train_loss", 0)
    _same_bits(arena_grads(explicit, src, tgt, z), arena_grads(default, src, tgt, z), cid)
    assert explicit.handle.get_counter("train_inbatch_steps") == 0


def test_inbatch_loss_falls_and_tracks_a_free_running_float64_reference():
    """60 steps on the toy batch of tests/test_gpu_train.py::test_several_steps_track_oracle_and_loss_falls (one batch of 32
    pair rows, lr 0.05), the device against float64 gradients + float64 clip and Adagrad run freely from the same initial weights.
    The loss falls on both sides; the final variables lie within 2e-2 of the reference's, the bar
    tests/test_gpu_trained_parity.py holds the variables of a free-running pair to.  (The loss itself falls by three orders of
    magnitude here, so its trajectory is printed, not held: two free runs reach the floor some steps apart.)"""
    from tests.util import make_pair, model_params, random_ids
    params = model_params("dual-encoder", 200, 50, 96, 96, 64, 12, lr=0.05)
    m, p = make_pair(params, seed=5)
    h = m.handle
    h.learning_rate = 0.05
    h.set_option("train_loss", 1)
    rng = np.random.RandomState(2)
    src = np.repeat(random_ids(rng, 16, 12, 200, 0.6), 2, axis=0)
    tgt = random_ids(rng, 32, 12, 200, 0.6)
    z = np.tile(np.array([1.0, 0.0], np.float32), 16)
    names = [n for n, _, _, _ in h.variables()]
    v = {n: np.asarray(p[n], np.float64) for n in names}
    slots = {n: np.full(v[n].shape, 0.1, np.float64) for n in names}
    start = m.get_variables(with_slots=True)
    for n in names:
        assert np.array_equal(start[n + "/Adagrad"].reshape(-1), np.full(v[n].size, 0.1, np.float32)), n
    got, want = [], []
    for _ in range(60):
        g, tail, _ = IC.step_reference(v, params, src, tgt, z)
        want.append(float(tail[1]))
        v, slots = reference_apply(g, tail, v, slots, 0.05)
        got.append(m.train_step(src, tgt, z)[0])
    got, want = np.array(got), np.array(want)
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-3)
    after = m.get_variables()
    dv = {n: float(np.abs(after[n].reshape(v[n].shape) - v[n]).max()) for n in names}
    print("INBATCH LEARN loss %.4f -> %.4f (float64 %.4f -> %.4f), max rel loss diff per 20 steps %s; max |device - float64| per variable %s"
          % (got[0], got[-1], want[0], want[-1], ["%.1e" % rel[i:i + 20].max() for i in range(0, 60, 20)],
             {n.split("/")[-1]: "%.1e" % d for n, d in dv.items()}))
    assert got[-1] < got[0] and want[-1] < want[0]
    for n, d in dv.items():
        assert d < 2e-2, (n, d)
    assert h.get_counter("train_inbatch_steps") == 60
