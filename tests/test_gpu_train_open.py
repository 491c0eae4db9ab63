"""The open train step (sse_train_forward* -> sse_train_backward_dev | sse_train_backward_inbatch_global) on the fused, any-shape
and text-CNN paths, by ids and by corpus rows, with and without a free target matrix.

The yardstick is sse_train_grads under train_loss = 1, train_pair_dedup = 0 on the same batch: an open step that takes its
gradients from the public sse_inbatch_loss_dev over its own encodings (keys built on the host, tests/inbatch_cases._row_keys),
or that is closed by the global head at world = 1, queues the same kernels on the same data.  So every gradient that
tests/test_gpu_train_state.py treats as reduced in a fixed order (all but the two lookup tables, ATOMIC there) and tail[0] must
agree bit for bit; the lookup tables within util.GRAD_BARS_EXACT.  The loss and accuracy the caller adds up on the host
(sse_train_backward_dev) are held to util.LOSS_REL_EXACT; the global closing reduces them on the device as the step does: bits."""
import ctypes as C

import numpy as np
import pytest

from tests import inbatch_cases as IC
from tests.test_gpu_train_state import ATOMIC
from tests.util import GRAD_BARS_EXACT, LOSS_REL_EXACT, arena_grads, check_grads, split_arena

pytestmark = pytest.mark.gpu

CASES = ("dual-unpaired-b40", "dual-paired-b128", "by-rows-equal-tokens", "seo-b40", "generic-forced", "cnn-b10")
PATH_COUNTER = {"fused": "train_path_fused", "generic": "train_path_generic", "cnn": "train_path_cnn"}
DEV = "cuda:0"


def _model(c, p, params, inbatch=False):
    import sse_amd
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    for k, v in c["opts"].items():
        m.handle.set_option(k, v)
    m.handle.set_option("train_loss_scale", c["scale"])
    if inbatch:
        m.handle.set_option("train_loss", 1)
        m.handle.set_option("train_pair_dedup", 0)
    return m


def _batch(c, m, src, tgt):
    """What the entry points take: the batch itself, or -- by_rows -- row numbers into uploaded, shuffled corpora."""
    if not c["by_rows"]:
        return src, tgt
    order = np.random.RandomState(5).permutation(len(src)).astype(np.int32)
    inv = np.argsort(order).astype(np.int32)
    m.handle.corpus_upload(0, src[order])
    m.handle.corpus_upload(1, tgt[order])
    return inv, inv


def _bind_nan_arena(h):
    import torch
    arena = torch.full((h.train_grad_count(),), float("nan"), dtype=torch.float32, device=DEV)
    h.train_bind_arena(arena)
    return arena


def _forward(c, h, a, b, z, rows_global):
    (h.train_forward_rows if c["by_rows"] else h.train_forward)(a, b, z, rows_global)


def _close_with_own_gradients(c, m, src, tgt, z, rows_global):
    """forward -> open encodings -> sse_inbatch_loss_dev with host-built keys -> sse_train_backward_dev."""
    import torch
    h = m.handle
    B, S = len(z), c["S"]
    arena = _bind_nan_arena(h)
    a, b = _batch(c, m, src, tgt)
    _forward(c, h, a, b, z, rows_global)
    st = torch.cuda.current_stream().cuda_stream
    raw = [torch.full((B, S), float("nan"), device=DEV) for _ in range(2)]
    for side in range(2):
        h.train_open_encodings(side, raw[side], st)
    ks, kt = (torch.tensor(IC._row_keys(x), dtype=torch.int64, device=DEV) for x in (src, tgt))
    d = [torch.full((B, S), float("nan"), device=DEV) for _ in range(2)]
    row_loss, row_acc = (torch.full((B,), float("nan"), device=DEV) for _ in range(2))
    h.inbatch_loss_dev(raw[0], raw[1], torch.tensor(z, device=DEV), ks, kt, B, S, float(c["scale"]), 1.0 / rows_global, d[0], d[1],
                       row_loss, row_acc, st)
    loss_part = float(row_loss.double().sum()) / rows_global
    acc_part = float(row_acc.double().sum()) / rows_global
    h.train_backward(d[0], d[1], loss_part, acc_part)
    torch.cuda.synchronize()
    return split_arena(m, arena.cpu().numpy())


def _close_global_one_rank(c, m, src, tgt, z, rows_global, pad=3):
    """forward -> pack -> (the gather of one rank: the block itself) -> sse_train_backward_inbatch_global, world = 1."""
    import torch
    h = m.handle
    arena = _bind_nan_arena(h)
    a, b = _batch(c, m, src, tgt)
    _forward(c, h, a, b, z, rows_global)
    cap = len(z) + pad
    block = torch.full((h.train_exchange_floats(cap, c["T"]),), float("nan"), device=DEV)
    h.train_pack_exchange(cap, block)
    h.train_backward_inbatch_global(block, 1, cap, 0, [len(z)])
    torch.cuda.synchronize()
    return split_arena(m, arena.cpu().numpy()), block.cpu().numpy()


def _same_fixed_order_bits(got, ref, what, tail_words):
    for n in ref[0]:
        assert not np.isnan(got[0][n]).any(), (what, n)
        if n not in ATOMIC:
            assert np.array_equal(got[0][n].view(np.uint32), ref[0][n].view(np.uint32)), "%s: %s differs in its bits" % (what, n)
    for i in tail_words:
        assert got[1][i:i + 1].view(np.uint32) == ref[1][i:i + 1].view(np.uint32), "%s: tail[%d] %r / %r" % (what, i, got[1][i], ref[1][i])
    want = {n: ref[0][n].astype(np.float64) for n in ATOMIC if n in ref[0]}
    check_grads(got[0], want, GRAD_BARS_EXACT, what=what + ": ")


@pytest.mark.parametrize("cid", CASES)
def test_open_step_equals_the_inbatch_step(cid):
    c = IC.STEP_CASES_BY_ID[cid]
    params, p = IC.step_params(c)
    src, tgt, z = IC.step_batch(c)
    rows_global = c["rows_factor"] * len(z)
    ref_model = _model(c, p, params, inbatch=True)
    ref = arena_grads(ref_model, *_batch(c, ref_model, src, tgt), z, rows_global, rows=c["by_rows"])
    assert ref_model.handle.get_counter("train_inbatch_steps") == 1 and ref_model.handle.get_counter("train_paired_steps") == 0

    # closed with the caller's own gradients (the options of the objective at their defaults: they are not consulted)
    m = _model(c, p, params)
    h = m.handle
    got = _close_with_own_gradients(c, m, src, tgt, z, rows_global)
    _same_fixed_order_bits(got, ref, cid + " own gradients", tail_words=(0, 3))
    assert abs(got[1][1] - ref[1][1]) <= LOSS_REL_EXACT * abs(ref[1][1]) + 1e-7, (got[1][1], ref[1][1])
    assert abs(got[1][2] - ref[1][2]) <= 1e-6, (got[1][2], ref[1][2])
    for path, counter in PATH_COUNTER.items():
        assert h.get_counter(counter) == (1 if path == c["path"] else 0), counter
    assert (h.get_counter("train_open_steps"), h.get_counter("train_global_inbatch_steps"), h.get_counter("train_inbatch_steps"),
            h.get_counter("train_paired_steps")) == (1, 0, 0, 0)
    assert h.train_apply() == (float(got[1][1]), float(got[1][2]))       # the closed step is a pending step like any other

    # closed by the global head at world = 1
    m = _model(c, p, params)
    h = m.handle
    got, block = _close_global_one_rank(c, m, src, tgt, z, rows_global)
    _same_fixed_order_bits(got, ref, cid + " global head, world 1", tail_words=(0, 1, 2, 3))
    assert (h.get_counter("train_open_steps"), h.get_counter("train_global_inbatch_steps"), h.get_counter("train_inbatch_steps"),
            h.get_counter("train_paired_steps")) == (1, 1, 0, 0)
    assert h.get_counter(PATH_COUNTER[c["path"]]) == 1
    # the block: the row count first, every pad slot zero, no word left unwritten
    B, S, T = len(z), c["S"], c["T"]
    cap = B + 3
    assert not np.isnan(block).any() and block[:1].view(np.int32)[0] == B
    Tt = 1 if c["mode"] in ("source-encoder-only", "source_only_cnn") else T
    assert block.size == 4 + cap * (2 * S + 1 + T + Tt)
    off = 4
    for width in (S, S, 1, T, Tt):
        sec = block[off:off + cap * width].reshape(cap, width)
        assert not sec[B:].view(np.uint32).any()
        off += cap * width
    assert np.array_equal(block[4 + 2 * cap * S:4 + 2 * cap * S + B], z)
    assert np.array_equal(block[4 + cap * (2 * S + 1):4 + cap * (2 * S + 1) + B * T].view(np.int32).reshape(B, T), src)
    assert np.array_equal(block[4 + cap * (2 * S + 1 + T):4 + cap * (2 * S + 1 + T) + B * Tt].view(np.int32).reshape(B, Tt),
                          np.asarray(tgt).reshape(B, Tt))


def _fresh_like(c, m, params):
    """A fresh handle with m's variables, slots and options."""
    return _model(c, m.get_variables(with_slots=True), params)


def _step_like_fresh(c, m, params, src, tgt, z, what):
    """sse_train_step on m and on a fresh handle with m's state: the same loss, accuracy and fixed-order variables, bit for bit."""
    fresh = _fresh_like(c, m, params)
    a, b = m.train_step(src, tgt, z), fresh.train_step(src, tgt, z)
    assert a == b, (what, a, b)
    va, vb = m.get_variables(with_slots=True), fresh.get_variables(with_slots=True)
    for n in va:
        if n.split("/Adagrad")[0] not in ATOMIC:
            assert np.array_equal(va[n].view(np.uint32), vb[n].view(np.uint32)), (what, n)


def _refused(fn, text, *args):
    import sse_amd
    with pytest.raises(sse_amd.SSEError, match=text):
        fn(*args)


def test_lifetime_rules_and_a_usable_handle_after_each_refusal():
    import torch
    c = IC.STEP_CASES_BY_ID["dual-unpaired-b40"]
    params, p = IC.step_params(c)
    src, tgt, z = IC.step_batch(c)
    B, S, T = len(z), c["S"], c["T"]
    m = _model(c, p, params)
    h = m.handle
    d = [torch.zeros((B, S), device=DEV) for _ in range(2)]
    cap = B
    block = torch.zeros(h.train_exchange_floats(cap, T), device=DEV)
    closings = {"backward": lambda: h.train_backward(d[0], d[1], 0.0, 0.0),
                "global": lambda: h.train_backward_inbatch_global(block, 1, cap, 0, [B])}
    n_open = 0

    def after(what):
        _step_like_fresh(c, m, params, src, tgt, z, what)

    # nothing open on a new handle
    for name, call in closings.items():
        _refused(call, "no step is open")
        after("no open step: " + name)
    _refused(h.train_pack_exchange, "no step is open", cap, block)
    _refused(h.train_open_encodings, "no step is open", 0, d[0])
    after("no open step: pack / encodings")
    # any other train step discards the open one
    for name, other in (("train_grads", lambda: h.train_grads(src, tgt, z)), ("train_step", lambda: m.train_step(src, tgt, z)),
                        ("eval does not", None)):
        h.train_forward(src, tgt, z)
        n_open += 1
        if other is None:
            h.eval_loss(src, tgt, z)                      # not a train step: the step stays open
            closings["backward"]()
            h.train_apply()
        else:
            other()
            _refused(closings["backward"], "no step is open")
        after("discarded by " + name)
    # a second forward replaces the first; one closing call, the second is refused
    h.train_forward(src[:8], tgt[:8], z[:8])
    h.train_forward(src, tgt, z)
    n_open += 2
    h.train_pack_exchange(cap, block)
    closings["global"]()
    for name, call in closings.items():
        _refused(call, "no step is open")
    h.train_apply()
    after("second closing call")
    # the variables changed
    name0, cnt0 = h.variables()[1][0], h.variables()[1][1]
    h.train_forward(src, tgt, z)
    n_open += 1
    h.set_variable(name0, h.get_variable(name0, cnt0))
    for call in closings.values():
        _refused(call, "the variables changed since sse_train_forward")
    _refused(h.train_pack_exchange, "the variables changed", cap, block)
    after("variables changed: set_variable")
    # (an update needs pending gradients, and whatever leaves them -- a train step or a closing call -- ends the open step first)
    # bad arguments of the plain calls; the step stays open through them and closes afterwards
    h.train_forward(src, tgt, z)
    n_open += 1
    _refused(h.train_pack_exchange, "cap = %d row slots, the open step holds %d rows" % (B - 1, B), B - 1, block)
    _refused(lambda: h.check(h.lib.sse_train_pack_exchange(h._h, cap, None)), "block must not be NULL")
    _refused(lambda: h.check(h.lib.sse_train_backward_dev(h._h, None, C.c_void_p(d[1].data_ptr()), 0.0, 0.0)), "must not be NULL")
    _refused(lambda: h.check(h.lib.sse_train_backward_dev(h._h, C.c_void_p(d[0].data_ptr()), None, 0.0, 0.0)), "must not be NULL")
    _refused(lambda: h.check(h.lib.sse_train_open_encodings_dev(h._h, 2, C.c_void_p(d[0].data_ptr()), None)), "bad arguments")
    _refused(h.train_apply, "no gradients pending")
    closings["backward"]()
    h.train_apply()
    after("bad arguments")
    assert h.get_counter("train_open_steps") == n_open and h.get_counter("train_global_inbatch_steps") == 1
    assert h.get_counter("train_paired_steps") == 0 and h.get_counter("train_inbatch_steps") == 0


GLOBAL_REFUSALS = [
    (dict(world=0, rows=[40]), r"world = 0, must be >= 1"),
    (dict(world=-2, rows=[40]), r"world = -2, must be >= 1"),
    (dict(rank=-1), r"rank -1 outside \[0, 2\)"),
    (dict(rank=2), r"rank 2 outside \[0, 2\)"),
    (dict(rows=[39, 41]), r"rank_rows\[0\] = 39, the open step of this rank holds 40 rows"),
    (dict(rows=[40, 45], rows_global=85), r"a rank holds 45 rows, more than the cap = 40 row slots"),
    (dict(rows=[40, 39]), r"rank_rows add up to 79 rows, the step was opened with rows_global = 80"),
    (dict(rows=[40, -1]), r"rank_rows\[1\] = -1 is negative"),
    (dict(null="gathered"), "must not be NULL"),
    (dict(null="rank_rows"), "must not be NULL"),
]


@pytest.mark.parametrize("kw,text", GLOBAL_REFUSALS, ids=[str(i) for i in range(len(GLOBAL_REFUSALS))])
def test_global_closing_refusals_leave_the_handle_usable(kw, text):
    import torch
    c = IC.STEP_CASES_BY_ID["dual-unpaired-b40"]
    params, p = IC.step_params(c)
    src, tgt, z = IC.step_batch(c)
    B, T = len(z), c["T"]
    m = _model(c, p, params)
    h = m.handle
    world, rank, rows = kw.get("world", 2), kw.get("rank", 0), kw.get("rows", [40, 40])
    h.train_forward(src, tgt, z, kw.get("rows_global", 80))
    gathered = torch.zeros(2 * h.train_exchange_floats(B, T), device=DEV)
    rr = np.asarray(rows, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    if kw.get("null") == "gathered":
        call = lambda: h.check(h.lib.sse_train_backward_inbatch_global(h._h, None, world, B, rank, ptr(rr)))
    elif kw.get("null") == "rank_rows":
        call = lambda: h.check(h.lib.sse_train_backward_inbatch_global(h._h, C.c_void_p(gathered.data_ptr()), world, B, rank, None))
    else:
        call = lambda: h.train_backward_inbatch_global(gathered, world, B, rank, rr)
    _refused(call, text)
    _refused(h.train_apply, "no gradients pending")          # nothing was queued, nothing is pending
    _step_like_fresh(c, m, params, src, tgt, z, text)


def test_batch_walk_40_8_40_equals_fresh_handles():
    """The buffers of the open step and of the global closing only grow: rows 8 .. 39 of a larger step must not reach a smaller
    one, on the fused and on the any-shape path."""
    for cid in ("dual-unpaired-b40", "generic-forced"):
        c0 = IC.STEP_CASES_BY_ID[cid]
        params, p = IC.step_params(c0)
        long_lived = _model(c0, p, params)
        for step, B in enumerate((40, 8, 40)):
            c = dict(c0, B=B, id="%s-walk-b%d" % (cid, B))
            src, tgt, z = IC.step_batch(c, seed=step)
            fresh = _model(c, p, params)
            a = _close_global_one_rank(c, long_lived, src, tgt, z, len(z), pad=step)[0]
            b = _close_global_one_rank(c, fresh, src, tgt, z, len(z), pad=step)[0]
            _same_fixed_order_bits(a, b, "%s step %d (B %d)" % (cid, step, B), tail_words=(0, 1, 2, 3))
