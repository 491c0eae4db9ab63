"""The train-step state a long-lived handle keeps from call to call -- TrainState of csrc/train_step.h: the two dirty flags of
the BPTT weight copies (ts.packed_dirty: KhT16 / KxT16, ts.fp32_dirty: KhT / KxT) beside h->packed_dirty / h->mp_fresh /
emb16_valid, the any-shape packs keyed by weights_version, the pair permutation with its permuted host copies, some forty
grow-only buffers whose rows B .. Bp and steps beyond T hold the previous batch, the resident corpora with corpus_N /
corpus_T, the gradient arena (internal / external, v.grad, grads_ready) and the side streams and events -- against a FRESH
handle (DESIGN "Per-handle training state").

One test per script of tests/train_state_script.py; each drives one long-lived handle through it.  Before every train call
the long-lived handle's variables and slots are copied into a fresh handle (get_variables(with_slots=True) ->
set_variables) that gets the same options and corpora; both run the call.  Then
  (a) loss, accuracy, tail[1..3] and every arena block named in BITWISE have the same bits on both handles (a fused step
      shows its arena only when an external one is bound; its loss and accuracy are compared either way).  BITWISE holds
      every variable whose gradient is reduced in a fixed order: all dense variables and tail[0].  Outside it are only the
      two lookup tables: word_embedding is scattered with float atomics by the dX stages (lstm_bwd2_kernel and
      lstm_bwd_kernel<.., X3> in-kernel dX, dx_kernel, gen_dx_scatter_kernel, cnn_dx_kernel / cnn_dx_mfma_kernel), the free
      target matrix by rows_scatter_kernel (see the docstring of test_train_step_by_rows_equals_train_step_by_ids).  A
      control at the start of each script runs the first train call on two fresh handles and asserts BITWISE between them:
      that proves the list, not the state;
  (b) the float64 oracle at util.GRAD_BARS_EXACT / GRAD_BARS_SPLIT and LOSS_REL_EXACT / LOSS_REL_SPLIT by the step's options
      -- the lookup tables are held here, and here only;
  (c) sse_train_apply against reference_apply of the device's own arena at 1e-6; for a fused step call against
      reference_apply of the FRESH handle's sse_train_grads arena of the same batch;
  (d) the deltas of the train_* counters against the model's expectation: path, paired, repacks;
  (e) refused and cancelled steps change nothing; an encode and an eval_loss between grads and apply leave the bound arena's
      bytes alone; an external arena that is no longer bound keeps its bytes.
(b) .. (e) are the runner's (tests/train_state_script.py, proven on the CPU by tests/test_train_state_host.py).  A failure
names the script, the step number, the options, the route and the steps before it.  One TRAINSTATE line per call
(profiles/train_state.txt)."""
import numpy as np
import pytest

from tests import train_state_script as TS
from tests.test_gpu_options_counters import COUNTERS as ALL_COUNTERS
from tests.util import make_pair, split_arena

pytestmark = pytest.mark.gpu

_LSTM = "/rnn/basic_lstm_cell/"
BITWISE = {
    "dual-encoder": ("source_encoder" + _LSTM + "kernel", "source_encoder" + _LSTM + "bias", "source_encoder/src_M",
                     "target_encoder" + _LSTM + "kernel", "target_encoder" + _LSTM + "bias", "target_encoder/tgt_M", "tail[0]"),
    "shared-encoder": ("shared_encoder" + _LSTM + "kernel", "shared_encoder" + _LSTM + "bias", "shared_encoder/src_M",
                       "shared_encoder/tgt_M", "tail[0]"),
    "source-encoder-only": ("source_only_encoder" + _LSTM + "kernel", "source_only_encoder" + _LSTM + "bias",
                            "source_only_encoder/src_M", "tail[0]"),
    "source_only_cnn": tuple("source_only_cnn/conv-maxpool-%d/%s" % (fs, x) for fs in (2, 3, 4, 5) for x in ("W", "b"))
                       + ("source_only_cnn/src_M", "tail[0]"),
}
ATOMIC = ("word_embedding", "target_embedding/tgt_seq_embedding")        # float atomics: the kernels are named above


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bitwise_differences(mode, a, b):
    """names of BITWISE (and tail[1..3]) whose bits differ between two (blocks, tail) arenas"""
    out = [n for n in BITWISE[mode] if n != "tail[0]" and not np.array_equal(_bits(a[0][n]), _bits(b[0][n]))]
    return out + ["tail[%d]" % i for i in range(4) if _bits(a[1])[i] != _bits(b[1])[i]]


class GpuDriver:
    """sse_amd's SSEModel / Handle behind the driver interface of the script"""

    def __init__(self, cfg, seed):
        import torch
        self.torch, self.cfg, self.mode = torch, cfg, cfg["network_mode"]
        self.m, p = make_pair(cfg, seed)
        self.m.set_variables({k + "/Adagrad": np.full(v.shape, TS.SLOT0, np.float32) for k, v in p.items()})
        self.h = self.m.handle
        self.opts, self.corpora = {}, {}
        self.ext, self.bound = {}, None
        self.atomic_moved = set()

    def close(self):
        self.h.close()

    @staticmethod
    def _guard(fn, *a, **kw):
        import sse_amd
        try:
            return fn(*a, **kw)
        except sse_amd.SSEError as e:
            raise TS.Refused(str(e))

    # -- state
    def _new_arena(self, h):
        return self.torch.full((h.train_grad_count(),), float("nan"), dtype=self.torch.float32, device="cuda:0")

    def set_option(self, name, v):
        self._guard(self.h.set_option, name, v)
        self.opts[name] = v

    def variables(self):
        return self.m.get_variables(with_slots=True)

    def set_variables(self, arrays):
        self.m.set_variables(arrays)

    def state(self):
        return dict(vars=self.variables(), global_step=self.h.global_step, counters={n: self.h.get_counter(n) for n in ALL_COUNTERS})

    def upload(self, side, ids):
        self._guard(self.h.corpus_upload, side, ids)
        self.corpora[side] = ids

    def bind_arena(self, kind):
        if kind is None:
            self.h.train_set_grad_arena(None, 0)
        else:
            if kind not in self.ext:
                self.ext[kind] = self._new_arena(self.h)
            self.h.train_bind_arena(self.ext[kind])
        self.bound = kind

    def arena_bytes(self, kind):
        if kind is None or kind not in self.ext:
            return b""
        self.torch.cuda.synchronize()
        return self.ext[kind].cpu().numpy().tobytes()

    def _counters(self):
        return {n: self.h.get_counter(n) for n in TS.TRAIN_COUNTERS}

    def _fresh(self):
        """a fresh handle holding the long-lived handle's variables, slots, options and corpora, a NaN arena bound"""
        import sse_amd
        f = sse_amd.SSEModel(self.cfg)
        f.set_variables(self.variables())
        f.handle.global_step = self.h.global_step
        for k, v in self.opts.items():
            f.handle.set_option(k, v)
        for side, ids in self.corpora.items():
            f.handle.corpus_upload(side, ids)
        arena = self._new_arena(f.handle)
        f.handle.train_bind_arena(arena)
        return f, arena

    def _read(self, model, arena):
        self.torch.cuda.synchronize()
        return split_arena(model, arena.cpu().numpy())

    @staticmethod
    def _grads(h, st):
        """sse_train_grads / sse_train_grads_rows of a train call (a fused step call: its gradient half)"""
        if st.kind in ("grads", "step"):
            h.train_grads(st.batch.src, st.batch.tgt, st.batch.z, rows_global=getattr(st, "rows_global", None))
        else:
            h.train_grads_rows(st.src_rows, st.tgt_rows, st.z, getattr(st, "rows_global", None) or len(st.z))

    # -- calls
    def call(self, st):
        k = st.kind
        if k in TS.TRAIN_CALLS:
            return self._train(st)
        c0 = self._counters()
        if k == "apply":
            loss, acc = self._guard(self.h.train_apply)
            return dict(loss=loss, acc=acc, vars=self.variables(), global_step=self.h.global_step, delta=self._delta(c0))
        f, _ = self._fresh()
        try:
            if k == "encode":
                side = 0 if st.side == "src" else 1
                got, want = self._guard(self.h.encode, side, st.ids), f.handle.encode(side, st.ids)
                assert np.array_equal(_bits(got), _bits(want)), "encodings differ from a fresh handle with the same variables"
                return dict(enc=got, delta=self._delta(c0))
            b = st.batch
            got, want = self._guard(self.h.eval_loss, b.src, b.tgt, b.z), f.handle.eval_loss(b.src, b.tgt, b.z)
            assert got == want, "eval_loss %r, a fresh handle's %r" % (got, want)
            return dict(loss=float(got[0]), acc=float(got[1]), delta=self._delta(c0))
        finally:
            f.handle.close()

    def _delta(self, c0):
        c1 = self._counters()
        return {n: c1[n] - c0[n] for n in c0}

    def _train(self, st):
        fused_step = st.kind in ("step", "step_rows")
        f, fa = self._fresh()
        try:
            own = self.bound is not None
            if own:
                self.ext[self.bound].fill_(float("nan"))
                self.torch.cuda.synchronize()
            c0 = self._counters()
            if st.kind == "step":
                loss, acc = self._guard(self.h.train_step, st.batch.src, st.batch.tgt, st.batch.z)
            elif st.kind == "step_rows":
                loss, acc = self._guard(self.h.train_step_rows, st.src_rows, st.tgt_rows, st.z)
            else:
                self._guard(self._grads, self.h, st)
            out = dict(delta=self._delta(c0))
            self._grads(f.handle, st)
            fresh = self._read(f, fa)
            if own:
                mine = self._read(self.m, self.ext[self.bound])
                bad = bitwise_differences(self.mode, mine, fresh)
                assert not bad, "differs from a fresh handle with the same variables, slots, options and corpora in %s" % bad
                self.atomic_moved.update(n for n in ATOMIC if n in mine[0] and not np.array_equal(_bits(mine[0][n]), _bits(fresh[0][n])))
            out.update(arena=fresh if (fused_step or not own) else mine, own=own)
            if fused_step:
                want = f.handle.train_apply()
                assert (loss, acc) == want, "(loss, acc) %r of the step, a fresh handle's %r" % ((loss, acc), want)
                out.update(loss=loss, acc=acc, vars=self.variables(), global_step=self.h.global_step)
            return out
        finally:
            f.handle.close()


def control(cfg, seed, steps, corpora):
    """The first train call of the script on two fresh handles: BITWISE must hold between them.  Returns the names of the
    atomically accumulated tables whose bits differed (for the record)."""
    first = next(st for st in steps if st.kind in TS.TRAIN_CALLS)
    arenas = []
    for _ in range(2):
        d = GpuDriver(cfg, seed)
        try:
            for side, ids in corpora.items():
                d.upload(side, ids)
            a = d._new_arena(d.h)
            d.h.train_bind_arena(a)
            d._grads(d.h, first)
            arenas.append(d._read(d.m, a))
        finally:
            d.close()
    bad = bitwise_differences(cfg["network_mode"], arenas[0], arenas[1])
    assert not bad, "control: two fresh handles differ in %s on %r" % (bad, first)
    return [n for n in ATOMIC if n in arenas[0][0] and not np.array_equal(_bits(arenas[0][0][n]), _bits(arenas[1][0][n]))]


@pytest.mark.parametrize("name", list(TS.SCRIPTS))
def test_train_state_script(name):
    for i, (cfg, seed, steps, marks) in enumerate(TS.SCRIPTS[name]()):
        label = name if i == 0 else "%s/%d" % (name, i + 1)
        first = next(j for j, st in enumerate(steps) if st.kind in TS.TRAIN_CALLS)
        corpora = {st.side: st.ids for st in steps[:first] if st.kind == "upload"}
        moved = control(cfg, seed, steps, corpora)
        d = GpuDriver(cfg, seed)
        try:
            r = TS.Runner(d, cfg, seed, name=label, out=print)
            r.run(steps)
            print(r.summary())
            print("TRAINSTATE %s BITWISE %s; atomically accumulated and seen to differ: control %s, script %s"
                  % (label, ", ".join(BITWISE[cfg["network_mode"]]), moved or "-", sorted(d.atomic_moved) or "-"))
            assert len(r.done) == len(steps)
        finally:
            d.close()
