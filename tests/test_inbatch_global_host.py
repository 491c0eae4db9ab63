"""The in-batch softmax loss over the GLOBAL batch of a data-parallel step, on the CPU.

(1) A numpy model of sse_train_backward_inbatch_global (NumpyOpenEngine below, built on tests/inbatch_cases.py and the
    oracle's forward / backward pieces): every rank encodes its own rows, packs them into a fixed-size block with pad slots,
    the blocks are "gathered", every rank compacts them in rank order, forms the keys over the GLOBAL id rows, runs the head
    over the global batch and keeps its window.  The ranks' arenas must add up to inbatch_cases.step_reference of the
    concatenated batch, within the bars of the step cases.  Five planted defects show that the check rejects each of them.
(2) Two `gloo` ranks: that engine behind the product's DataParallelTrainer(global_negatives=True); the updated variables equal
    ONE engine's in-batch step on the concatenated batch, and the default (local negatives) does not."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import sse_oracle as O
from tests import inbatch_cases as IC
from tests.rank_launch import free_port
from tests.test_distributed_gloo import OracleEngine
from tests.util import GRAD_BARS_EXACT, LOSS_REL_EXACT, check_grads, oracle_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFECTS = ("keys-per-rank", "window-off-by-one", "inv-rows-local", "pad-slots-as-columns", "rank-order-swapped")
CASE = IC._sc("global-host", "dual-encoder", 60, 8, 12, 12, 16, 6, 14, batch="unpaired")
SCALE = 64.0


class NumpyOpenEngine(OracleEngine):
    """The open train step of include/sse_hip.h in numpy, dual-encoder mode: train_forward, train_exchange_floats,
    train_pack_exchange, train_backward_inbatch_global; train_grads = the in-batch step with the rank's own rows as negatives
    (inbatch_cases.step_reference).  Arithmetic in float64, the arena in its own precision.  The block has the library's
    sections -- [rows, S, T, T | src raw | tgt raw | labels | src ids | tgt ids] over cap row slots, pad slots zeroed -- with the
    ids stored as values.  defect: one of DEFECTS, a planted error of the closing call."""

    def __init__(self, params, cfg, lr, defect=None):
        OracleEngine.__init__(self, params, cfg, lr)
        self.defect, self.open, self.scale = defect, None, SCALE
        self.S, self.T = int(cfg["encoding_size"]), int(cfg["max_seq_length"])

    def set_option(self, name, value):
        assert name == "train_loss_scale", name
        self.scale = float(value)

    # ---- the two halves of inbatch_cases._step_gradients
    def _encode(self, src, tgt):
        mode, F = self.cfg["network_mode"], O.F32
        p = {k: np.asarray(v, F) for k, v in self.p.items()}
        emb, fw = p["word_embedding"], {}
        for side, ids in (("src", src), ("tgt", tgt)):
            scope = O.lstm_scope(mode, side)
            K, b = p[scope + "/rnn/basic_lstm_cell/kernel"], p[scope + "/rnn/basic_lstm_cell/bias"]
            h, tape = O.lstm_forward(emb, K, b, ids, keep_tape=True)
            M = p[O.proj_name(mode, side)]
            fw[side] = dict(scope=scope, K=K, h=h, tape=tape, M=M, raw=(h @ M).astype(F), ids=O.check_ids(ids, emb.shape[0]))
        return fw

    def _backward(self, fw, d_src, d_tgt):
        mode, F = self.cfg["network_mode"], O.F32
        E = self.p["word_embedding"].shape[1]
        grads, sl_ids, sl_rows = {}, [], []
        for side, draw in (("src", d_src), ("tgt", d_tgt)):
            f = fw[side]
            grads[O.proj_name(mode, side)] = (f["h"].T @ draw).astype(F)
            dK, db, dX = O._lstm_backward(f["K"], f["tape"], (draw @ f["M"].T).astype(F), E)
            grads[f["scope"] + "/rnn/basic_lstm_cell/kernel"] = dK
            grads[f["scope"] + "/rnn/basic_lstm_cell/bias"] = db
            sl_ids.append(f["ids"].reshape(-1))
            sl_rows.append(dX.reshape(-1, E))
        grads["word_embedding"] = (np.concatenate(sl_ids), np.concatenate(sl_rows).astype(F))
        return grads

    def _fill_arena(self, grads, loss, acc, rows):
        off, sq = 0, 0.0
        for n in self.names:
            g = grads[n]
            if isinstance(g, tuple):
                sq += float(np.sum(np.square(g[1].astype(np.float64))))
                g = O.dense_embedding_grad(g, self.p[n].shape[0])
            self.arena[off:off + g.size] = np.asarray(g, np.float64).ravel()
            off += g.size
        self.arena[off:off + 4] = (sq, loss, acc, rows)

    # ---- the entry points DataParallelTrainer uses
    def train_grads(self, src, tgt, labels, rows_global):
        self.open = None
        dense, tail, _ = IC.step_reference(self.p, self.cfg, src, tgt, labels, rows_global, self.scale)
        off = 0
        for n in self.names:
            self.arena[off:off + dense[n].size] = dense[n].ravel()
            off += dense[n].size
        self.arena[off:off + 4] = tail

    def train_forward(self, src, tgt, labels, rows_global):
        with oracle_float64():
            fw = self._encode(np.asarray(src), np.asarray(tgt))
        self.open = dict(fw=fw, src=np.asarray(src), tgt=np.asarray(tgt), z=np.asarray(labels, np.float64), rows_global=int(rows_global))

    def train_exchange_floats(self, cap, T):
        assert T == self.T
        return 4 + cap * (2 * self.S + 1 + 2 * T)

    def _sections(self, buf, cap):
        S, T, off, out = self.S, self.T, 4, []
        for width in (S, S, 1, T, T):
            out.append(buf[off:off + cap * width].reshape(cap, width))
            off += cap * width
        return out

    def train_pack_exchange(self, cap, block):
        o = self.open
        buf = block.numpy() if hasattr(block, "numpy") else block
        B = len(o["z"])
        assert B <= cap and buf.size == self.train_exchange_floats(cap, self.T)
        buf[:] = 0                                                # pad slots zeroed
        buf[:4] = (B, self.S, self.T, self.T)
        for sec, a in zip(self._sections(buf, cap), (o["fw"]["src"]["raw"], o["fw"]["tgt"]["raw"], o["z"][:, None], o["src"], o["tgt"])):
            sec[:B] = a

    def train_backward_inbatch_global(self, gathered, world, cap, rank, rank_rows):
        o, self.open = self.open, None
        assert o is not None, "no step is open"
        buf = gathered.numpy() if hasattr(gathered, "numpy") else gathered
        rank_rows = [int(v) for v in rank_rows]
        B = len(o["z"])
        assert rank_rows[rank] == B and max(rank_rows) <= cap and sum(rank_rows) == o["rows_global"]
        n = self.train_exchange_floats(cap, self.T)
        taken = [cap] * world if self.defect == "pad-slots-as-columns" else rank_rows
        order = list(range(world))[::-1] if self.defect == "rank-order-swapped" else list(range(world))
        parts = []
        for r in order:                                           # compaction: global row = rows of the lower ranks + local row
            blk = buf[r * n:(r + 1) * n]
            assert int(blk[0]) == rank_rows[r]
            parts.append([np.asarray(sec[:taken[r]], np.float64) for sec in self._sections(blk, cap)])
        gs, gt, gz, gsrc, gtgt = (np.concatenate([p[k] for p in parts]) for k in range(5))
        gz = gz[:, 0]
        if self.defect == "keys-per-rank":                        # a repeat on another rank is not seen
            ks = np.concatenate([IC._row_keys(p[3]) + 1000 * i for i, p in enumerate(parts)])
            kt = np.concatenate([IC._row_keys(p[4]) + 1000 * i for i, p in enumerate(parts)])
        else:
            ks, kt = IC._row_keys(gsrc.astype(np.int64)), IC._row_keys(gtgt.astype(np.int64))
        inv = 1.0 / (B if self.defect == "inv-rows-local" else o["rows_global"])
        r = IC.head(gs, gt, gz, ks, kt, self.scale, inv)
        lo = sum(taken[:rank])
        win = np.arange(lo, lo + B)
        if self.defect == "window-off-by-one":
            win = (win + 1) % len(gz)
        with oracle_float64():
            grads = self._backward(o["fw"], r["d_src"][win], r["d_tgt"][win])
        self._fill_arena(grads, inv * r["row_loss"][win].sum(), inv * r["row_acc"][win].sum(), B)


# ---- (1) the numpy model ------------------------------------------------------------------------------------------------
def _global_batch(rows, seed):
    """Rank slices (src, tgt, z) with a source of rank 0 repeated on the last rank, both rows verified, and a target of rank 0
    repeated on rank 1; returns (slices, concatenation)."""
    parts = [list(IC.step_batch(dict(CASE, B=max(B, 2)), seed=seed + 10 * r)) for r, B in enumerate(rows)]
    parts = [[a[:B].copy() for a in part] for part, B in zip(parts, rows)]
    last = len(rows) - 1
    i0, j0 = 1 % rows[0], rows[last] - 1
    parts[last][0][j0] = parts[0][0][i0]                            # the same source on two ranks ...
    parts[0][2][i0] = parts[last][2][j0] = 1.0                      # ... with a verified target each
    parts[1][1][0] = parts[0][1][0]                                 # the same target on two ranks
    parts[1][2][0] = 1.0
    whole = tuple(np.concatenate([part[k] for part in parts]) for k in range(3))
    return parts, whole


def _seeded(rows):
    """The first batch seed that meets the accuracy precondition: min_accuracy_gap > accuracy_gap_bound on the global batch."""
    params, p = IC.step_params(CASE)
    for seed in range(32):
        parts, (src, tgt, z) = _global_batch(rows, seed)
        want, want_tail, r = IC.step_reference(p, params, src, tgt, z, len(z), SCALE)
        with oracle_float64():
            fw = NumpyOpenEngine(p, params, 0.9)._encode(src, tgt)
        gap = IC.min_accuracy_gap(fw["src"]["raw"], fw["tgt"]["raw"], z, IC._row_keys(src), IC._row_keys(tgt), SCALE)
        if gap > IC.accuracy_gap_bound(SCALE, CASE["S"]):
            return params, p, parts, (src, tgt, z), want, want_tail, r, gap
    raise AssertionError("no seed meets the accuracy precondition for rows %r" % (rows,))


def _run_ranks(params, p, parts, defect=None, pad=2):
    """Every rank's open step through the model; returns the SUM of the ranks' arenas as ({variable: gradient}, tail)."""
    rows = [len(part[2]) for part in parts]
    world, cap, G = len(rows), max(rows) + pad, sum(rows)
    engines, blocks = [], []
    for part in parts:
        e = NumpyOpenEngine({k: np.asarray(v, np.float64) for k, v in p.items()}, params, 0.9, defect)
        e.arena = np.zeros(e.train_grad_count(), np.float64)
        e.train_forward(part[0], part[1], part[2], G)
        block = np.full(e.train_exchange_floats(cap, CASE["T"]), np.nan)
        e.train_pack_exchange(cap, block)
        assert not np.isnan(block).any()
        engines.append(e)
        blocks.append(block)
    gathered = np.concatenate(blocks)
    total = np.zeros_like(engines[0].arena)
    for rank, e in enumerate(engines):
        e.train_backward_inbatch_global(gathered, world, cap, rank, rows)
        total += e.arena
    out, off = {}, 0
    for n in engines[0].names:
        out[n] = total[off:off + p[n].size].reshape(p[n].shape)
        off += p[n].size
    return out, total[off:]


ROWS = ((5, 9), (1, 32, 7))


@pytest.mark.parametrize("rows", ROWS, ids=["5+9", "1+32+7"])
def test_rank_windows_of_the_global_head_add_up_to_the_single_rank_step(rows):
    params, p, parts, (src, tgt, z), want, want_tail, r, gap = _seeded(rows)
    assert gap > IC.accuracy_gap_bound(SCALE, CASE["S"])
    # the planted repeats are in the batch and they matter: a key formed per rank would admit columns the global key excludes
    ks, kt = IC._row_keys(src), IC._row_keys(tgt)
    lo_last = sum(rows[:-1])
    assert (ks[lo_last:] < rows[0]).any() and (kt[rows[0]:rows[0] + rows[1]] < rows[0]).any()
    got, tail = _run_ranks(params, p, parts)
    errs = IC.check_step(got, tail, want, want_tail, CASE, what="rows %r: " % (rows,))
    print("GLOBAL HOST rows %r: gap %.3g (bound %.3g); norm %.2e element %.2e" % (
        rows, gap, IC.accuracy_gap_bound(SCALE, CASE["S"]), max(e[0] for e in errs.values()), max(e[1] for e in errs.values())))


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("rows", ROWS, ids=["5+9", "1+32+7"])
def test_planted_defects_are_rejected(rows, defect):
    params, p, parts, _, want, want_tail, _, _ = _seeded(rows)
    got, tail = _run_ranks(params, p, parts, defect=defect)
    with pytest.raises(AssertionError):
        IC.check_step(got, tail, want, want_tail, CASE, what="%s: " % defect)


# ---- (2) two gloo ranks behind the product's DataParallelTrainer -------------------------------------------------------------
def _worker(rank, world, port, out_dir, rows, global_negatives):
    sys.path.insert(0, ROOT)
    os.environ["SSE_NO_TORCH"] = "1"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sse_amd
    params, p, parts = _seeded(rows)[:3]
    eng = NumpyOpenEngine({k: np.array(v, np.float32) for k, v in p.items()}, params, 0.9)
    tr = sse_amd.DataParallelTrainer(eng, options={"train_loss_scale": int(SCALE)}, global_negatives=global_negatives)
    loss, acc = tr.train_step(*parts[rank])                       # uneven rows: the counts come from the tiny all-gather
    np.savez(os.path.join(out_dir, "g%d_rank%d.npz" % (int(global_negatives), rank)), hist=np.array([loss, acc]), **eng.p)
    dist.barrier()
    dist.destroy_process_group()


def _one_engine(params, p, src, tgt, z):
    eng = NumpyOpenEngine({k: np.array(v, np.float32) for k, v in p.items()}, params, 0.9)
    eng.train_bind_arena(torch.zeros(eng.train_grad_count(), dtype=torch.float32))
    eng.train_grads(src, tgt, z, len(z))
    return eng.train_apply(), eng.p


def test_two_gloo_ranks_with_global_negatives_equal_one_engine_on_the_concatenated_batch(tmp_path):
    rows = ROWS[0]
    params, p, parts, (src, tgt, z) = _seeded(rows)[:4]
    (loss, acc), after = _one_engine(params, p, src, tgt, z)
    names = sorted(after)
    before = {n: np.asarray(p[n], np.float64) for n in names}
    want = {n: after[n].astype(np.float64) for n in names}
    moved_want = {n: want[n] - before[n] for n in names}
    assert all(np.abs(moved_want[n]).max() > 0 for n in names)
    for global_negatives in (True, False):
        mp.spawn(_worker, args=(2, free_port(), str(tmp_path), rows, global_negatives), nprocs=2, join=True)
        out = [np.load(os.path.join(str(tmp_path), "g%d_rank%d.npz" % (int(global_negatives), r))) for r in range(2)]
        for n in names:
            assert np.array_equal(out[0][n], out[1][n]), n         # the ranks stay in lock-step, bit for bit
        got = {n: out[0][n].astype(np.float64) for n in names}
        moved = {n: got[n] - before[n] for n in names}
        if global_negatives:
            check_grads(got, want, GRAD_BARS_EXACT, what="variables after the step: ")
            check_grads(moved, moved_want, GRAD_BARS_EXACT, what="the update itself: ")
            for r in range(2):
                assert abs(out[r]["hist"][0] - loss) <= LOSS_REL_EXACT * abs(loss) + 1e-7 and abs(out[r]["hist"][1] - acc) <= 1e-6
        else:                                                       # the rank's own rows as negatives: another objective
            with pytest.raises(AssertionError):
                check_grads(moved, moved_want, GRAD_BARS_EXACT, what="local negatives: ")


def test_an_engine_without_the_open_step_is_refused():
    import sse_amd
    params, p = IC.step_params(CASE)
    eng = OracleEngine({k: np.array(v, np.float32) for k, v in p.items()}, params, 0.9)
    with pytest.raises(ValueError, match="global_negatives=True needs an engine with the open train step"):
        sse_amd.DataParallelTrainer(eng, global_negatives=True)


def test_one_rank_with_an_even_split_takes_its_row_counts_from_shard_bounds():
    """rows_global passed, no process group: world 1, the block gathered by a copy; equals the engine's own in-batch step."""
    import sse_amd
    params, p, parts, (src, tgt, z) = _seeded(ROWS[0])[:4]
    (loss, acc), want = _one_engine(params, p, src, tgt, z)
    eng = NumpyOpenEngine({k: np.array(v, np.float32) for k, v in p.items()}, params, 0.9)
    tr = sse_amd.DataParallelTrainer(eng, global_negatives=True)
    got = tr.train_step(src, tgt, z, rows_global=len(z))
    assert abs(got[0] - loss) <= LOSS_REL_EXACT * abs(loss) + 1e-7 and abs(got[1] - acc) <= 1e-6
    check_grads({n: eng.p[n].astype(np.float64) for n in want}, {n: want[n].astype(np.float64) for n in want}, GRAD_BARS_EXACT)
