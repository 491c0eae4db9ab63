"""The train step's caller buffers on guarded, skewed placements (tests/guard_bands.py): the gradient arena bound with
train_bind_arena, the packed buffer of sse_train_pack_embedding_grad and the gathered buffer of
sse_train_unpack_embedding_grad sit between guards, with no skew and one element off 16-byte alignment, under both fills.

One small existing case per path of tests/test_gpu_train_grads.py (fused, train_gen1, x3-111, generic-h33-129, seo-h128, cnn,
cnn-bf16), one in-batch step of tests/inbatch_cases.py and one class-loss step of tests/class_loss_cases.py (dense d_table).
Every call runs on a fresh handle with the case's weights, so the whole-allocation call and the two fills compute the same
step: the gradients are held with check_grads / check_tail at the case's bars as today, the tail and every variable outside
tests/test_gpu_train_state.py::ATOMIC (the two lookup tables, scattered with float atomics) must be bit-identical between the
three, and the guards are checked twice -- after sse_train_grads and again after sse_train_apply."""
import numpy as np
import pytest

from tests import class_loss_cases as CL
from tests import guard_bands as GB
from tests import inbatch_cases as IC
from tests import test_gpu_train_grads as TG
from tests.test_gpu_train_state import ATOMIC
from tests.util import LOSS_REL_EXACT, LOSS_REL_SPLIT, check_grads, check_tail, reference_grads, split_arena

pytestmark = pytest.mark.gpu
F32 = np.float32
GRADS_CASES = ("e32", "gen1-shared96", "x3-111", "generic-h33-129", "seo-h128", "cnn", "cnn-bf16")   # e32: the fused path
PATHS = ("train_path_fused", "train_path_generic", "train_path_cnn")


def _arena_spec(count):
    """the flat arena has no rows to round: each guard is as large as the arena itself, never under 64 KiB"""
    return GB.spec(F32, count, "out", guard=GB.round_up(max(count * 4, GB.MIN_GUARD), GB.ALIGN))


def _tg_case(cid):
    return next(c.values[0] for c in TG.CASES if c.values[0]["id"] == cid)


def _sync():
    import torch
    torch.cuda.synchronize()


def _setup(cid):
    """(new model, src, tgt, z, rows_global, check(blocks, tail), counters expected to read 1 after one step)"""
    if cid in GRADS_CASES:
        c = _tg_case(cid)
        params, p = TG.case_params(c)
        src, tgt, z = TG.case_batch(c)
        TG.cnn_preconditions(c, p, src)
        rows_global = c["rows_factor"] * len(z)
        want, want_tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=bool(c["opts"].get("cnn_bf16")))
        bars = TG.case_bars(c)

        def check(got, tail, what):
            check_grads(got, want, bars, what=what, var_bars=c.get("var_bars"))
            check_tail(tail, want_tail, bars, LOSS_REL_SPLIT if c["opts"].get("train_fwd_x3") else LOSS_REL_EXACT)
        return (lambda: TG._model(c)[1]), src, tgt, z, rows_global, check, (("train_path_cnn",) if cid.startswith("cnn") else ())
    if cid == "inbatch":
        from tests.test_gpu_inbatch_train import _model
        c = IC.STEP_CASES_BY_ID["dual-unpaired-b40"]
        params, p, src, tgt, z, want, want_tail, _ = IC.step_case_seeded(c)
        return (lambda: _model(c, p, params)), src, tgt, z, len(z), (lambda got, tail, what: IC.check_step(got, tail, want, want_tail, c, what)), \
            ("train_path_fused", "train_inbatch_steps")
    from tests.test_gpu_class_train import _model
    c = CL.STEP_CASES_BY_ID["seo-fused-b70-n40"]
    params, p, src, tgt, z, want, want_tail, _ = CL.step_case_seeded(c)
    return (lambda: _model(c, p, params)), src, tgt, z, len(z), (lambda got, tail, what: CL.check_step(got, tail, want, want_tail, c, what)), \
        ("train_path_fused", "train_class_steps")


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("cid", GRADS_CASES + ("inbatch", "class"))
def test_train_grads_and_apply_into_a_guarded_arena(cid, skew):
    new_model, src, tgt, z, rows_global, check, counters = _setup(cid)
    count = new_model().handle.train_grad_count()
    snaps = []

    def call(b):
        m = new_model()
        h = m.handle
        h.train_bind_arena(b["arena"].tensor())
        h.train_grads(src, tgt, z, rows_global=rows_global)
        _sync()
        flat = b["arena"].verify()                      # the guards after sse_train_grads (raises), and the raw gradients
        assert sum(h.get_counter(name) for name in PATHS) == 1          # one step, on one path
        for name in counters:
            assert h.get_counter(name) == 1, name
        got, tail = split_arena(m, flat)
        assert not np.isnan(flat).any(), "an element of the arena was not written"
        check(got, tail, "%s skew %d fill %s: " % (cid, skew, b["arena"].fill))
        snaps.append((got, tail))
        loss, acc = h.train_apply()                     # the guards after sse_train_apply: checked by the harness
        assert (loss, acc) == (float(tail[1]), float(tail[2]))
        _sync()
        return loss, acc
    calls = GB.run_guarded.calls
    # (what sse_train_apply leaves in the arena is not specified: the bit comparison below is on the gradients before it)
    GB.drive(GB.TorchBackend(), dict(arena=_arena_spec(count)), call, skew, compare=dict(arena=lambda *a: None))
    assert len(snaps) == 3                              # whole allocation, fill ones, fill valid
    for got, tail in snaps[1:]:
        assert GB.same_bits(tail, snaps[0][1]), "tail %r / %r" % (tail, snaps[0][1])
        for name in got:
            if name not in ATOMIC or cid == "class" and name == CL.TABLE:       # (a class step's table gradient is dense: no atomics)
                assert GB.same_bits(np.ascontiguousarray(got[name]), np.ascontiguousarray(snaps[0][0][name])), \
                    "%s: %s differs from the whole-allocation call" % (cid, name)
    print("GUARDCALLS train %d" % (GB.run_guarded.calls - calls))


class _Ptr(object):
    """what Handle.dp_pack_embedding / dp_unpack_embedding take: anything with a data_ptr()"""

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def _exchange_case():
    c = _tg_case("e32")
    params, p = TG.case_params(c)
    src, tgt, z = TG.case_batch(c)
    return c, params, p, src, tgt, z


def _canonical(packed, cap, E):
    """(count, header words 1 .. 3, ids ascending, their rows): the slots are taken in no fixed order (atomic counter), the set is"""
    words = packed.view(np.int32)
    n = min(int(words[0]), cap)
    cap4 = (cap + 3) & ~3
    ids = words[4:4 + n].copy()
    rows = packed[4 + cap4:4 + cap4 + cap * E].reshape(cap, E)[:n]
    o = np.argsort(ids, kind="stable")
    return int(words[0]), words[1:4].tolist(), ids[o], rows[o]


@pytest.mark.parametrize("skew", (0, 1))
def test_pack_embedding_grad_into_a_guarded_buffer_exact_cap_and_one_short(skew):
    import sse_amd
    c, params, p, src, tgt, z = _exchange_case()
    V, E = c["V"], c["E"]
    touched = np.unique(np.concatenate([src.ravel(), tgt.ravel()]))
    be = GB.TorchBackend()
    calls = GB.run_guarded.calls
    state = {}

    def specs(cap, m):
        n = m.handle.dp_packed_floats(cap)
        assert n == 4 + ((cap + 3) & ~3) + cap * E
        # valid fill 0.0f: as a slot word an in-range row, as a gradient a value
        return dict(arena=_arena_spec(m.handle.train_grad_count()),
                    packed=GB.spec(F32, n, "out", valid=0.0, guard=GB.guard_bytes(GB.round_up(cap, 64), E, 4, 64, 64)))

    def run(cap, expect_error):
        def call(b):
            m = TG._model(c)[1]
            h = m.handle
            h.train_bind_arena(b["arena"].tensor())
            h.train_grads(src, tgt, z)
            h.dp_pack_embedding(cap, _Ptr(b["packed"].ptr))
            _sync()
            dense = b["arena"].verify()[:V * E].reshape(V, E)
            state["dense"], state["packed"] = dense, b["packed"].verify()
            if not expect_error:
                h.train_apply()
                return "ok"
            with pytest.raises(sse_amd.SSEError, match="embedding-gradient exchange"):      # device error bit 8
                h.train_apply()
            after = m.get_variables()
            assert all(np.array_equal(np.asarray(p[k], F32).reshape(after[k].shape), after[k]) for k in p), "the update was not cancelled"
            return "bit 8"

        def same_set(name, a, b):
            ca, cb = _canonical(a, cap, E), _canonical(b, cap, E)
            assert ca[0] == cb[0] and ca[1] == cb[1]
            if ca[0] <= cap:                            # (on an overflow WHICH rows found a slot is not determined)
                assert np.array_equal(ca[2], cb[2])      # (the rows are the embedding gradient: ATOMIC, held against the arena below)
        m0 = TG._model(c)[1]
        GB.drive(be, specs(cap, m0), call, skew, compare=dict(arena=lambda *a: None, packed=same_set))
    # the rows that carry a gradient: found with a roomy cap first
    run(len(touched), False)
    rows = np.flatnonzero((state["dense"] != 0).any(axis=1))
    cap = len(rows)
    assert 0 < cap <= len(touched)
    run(cap, False)                                     # cap == the rows touched: the last slot is used, nothing behind it
    count, zeros, ids, grads = _canonical(state["packed"], cap, E)
    assert count == cap and zeros == [0, 0, 0] and np.array_equal(ids, rows)
    assert GB.same_bits(np.ascontiguousarray(grads), np.ascontiguousarray(state["dense"][rows]))
    run(cap - 1, True)                                  # one slot short: flagged, cancelled, and nothing written past the buffer
    assert _canonical(state["packed"], cap - 1, E)[0] == cap
    print("GUARDCALLS train %d" % (GB.run_guarded.calls - calls))


@pytest.mark.parametrize("skew", (0, 1))
def test_unpack_embedding_grad_from_a_guarded_gathered_buffer_of_two_ranks(skew):
    c, params, p, src, tgt, z = _exchange_case()
    V, E, cap = c["V"], c["E"], 37
    cap4 = (cap + 3) & ~3
    n = 4 + cap4 + cap * E
    rng = np.random.RandomState(3)
    gathered = np.zeros(2 * n, F32)
    want = np.zeros((V, E), F32)
    for r, count in enumerate((cap, 5)):                # rank 0 fills every slot, rank 1 five of them; they share rows
        buf = gathered[r * n:(r + 1) * n]
        ids = np.sort(rng.choice(V - 1, size=count, replace=False)).astype(np.int32)
        if r == 1:
            ids[0] = V - 1                               # the last row of the table
        rows = rng.standard_normal((count, E)).astype(F32)
        buf.view(np.int32)[0] = count
        buf.view(np.int32)[4:4 + count] = ids
        buf[4 + cap4:4 + cap4 + count * E] = rows.ravel()
        buf[4 + cap4 + count * E:] = 7.0                 # unused slots of a gathered buffer: never read
        want[ids] = want[ids] + rows                     # rank order
    m0 = TG._model(c)[1]
    count = m0.handle.train_grad_count()
    specs = dict(arena=_arena_spec(count),
                 gathered=GB.spec(F32, 2 * n, "in", init=gathered, valid=0.0, guard=GB.guard_bytes(2 * GB.round_up(cap, 64), E, 4, 64, 64)))

    def call(b):
        m = TG._model(c)[1]
        h = m.handle
        h.train_bind_arena(b["arena"].tensor())
        h.train_grads(src, tgt, z)
        _sync()
        before = b["arena"].verify()
        h.dp_unpack_embedding(_Ptr(b["gathered"].ptr), 2, cap)
        _sync()
        after = b["arena"].verify()
        assert GB.same_bits(np.ascontiguousarray(after[:V * E].reshape(V, E)), want), "the dense block is not rank 0 + rank 1"
        assert GB.same_bits(after[V * E:], before[V * E:]), "the arena behind the dense block moved"
        return h.train_apply()                           # no error bit: every id was in range
    calls = GB.run_guarded.calls
    GB.drive(GB.TorchBackend(), specs, call, skew, compare=dict(arena=lambda *a: None))
    print("GUARDCALLS train %d" % (GB.run_guarded.calls - calls))
