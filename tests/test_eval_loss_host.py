"""Host side of the forward-only loss, no GPU: Data.get_eval_pairs on the rawdata-qna fixture, and
DataParallelTrainer.eval_loss as two gloo ranks with the numpy oracle as the engine."""
import os
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

import sse_amd  # noqa: F401
from sse_amd import sse_data
from tests.rank_launch import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
RAW_QNA = os.path.join(G, "rawdata-qna")
T = 40


def _data(work, seed):
    return sse_data.Data(work, RAW_QNA, 8000, T, seed=seed, log=lambda *a: None)


def test_get_eval_pairs_layout_and_negatives(tmp_path):
    d = _data(str(tmp_path), 3)
    n = len(d.rawEvalCorpus)
    assert n > 0
    src, tgt, labels = d.get_eval_pairs(seed=0)
    assert src.shape == tgt.shape == (2 * n, T) and src.dtype == tgt.dtype == np.int32
    assert labels.dtype == np.float32 and labels.tolist() == [1.0, 0.0] * n
    _, rows, _ = d.get_eval_pairs(seed=0, target_rows=True)
    assert rows.shape == (2 * n,) and rows.dtype == np.int32
    tgt_corpus = d.corpus_matrices()[1]
    assert np.array_equal(tgt_corpus[rows], tgt)
    for i, (tokens, verified) in enumerate(d.rawEvalCorpus):
        assert src[2 * i].tolist() == src[2 * i + 1].tolist() == list(tokens)
        positives = set(d.target_row(t) for t in verified)
        assert rows[2 * i] == d.target_row(verified[0])               # the first verified target
        assert rows[2 * i + 1] not in positives                       # a negative is none of the row's positives
    assert len(set(rows[1::2].tolist())) > 1                          # ... and they are drawn, not one fixed row
    # the same seed gives the same pairs (also from the 'compressed' cache of a second Data), another seed other negatives
    again = _data(str(tmp_path), 11).get_eval_pairs(seed=0, target_rows=True)
    assert np.array_equal(again[0], src) and np.array_equal(again[1], rows) and np.array_equal(again[2], labels)
    other = d.get_eval_pairs(seed=1, target_rows=True)[1]
    assert np.array_equal(other[0::2], rows[0::2]) and not np.array_equal(other[1::2], rows[1::2])


def test_get_eval_pairs_leaves_the_training_stream_alone(tmp_path):
    a, b = _data(str(tmp_path), 5), _data(str(tmp_path), 5)
    for step in range(4):
        if step in (0, 2):
            b.get_eval_pairs(seed=step)
        x, y = a.get_train_batch_rows(6), b.get_train_batch_rows(6)
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
        b.get_eval_pairs(seed=0, target_rows=True)
        assert a.get_train_batch(3) == b.get_train_batch(3)


# ---- DataParallelTrainer.eval_loss: two gloo ranks, the oracle as the engine ----------------------------------------
def _dp_cfg():
    from util import model_params
    return model_params("dual-encoder", 60, 8, 12, 16, 16, 6)


def _dp_batch(rows):
    rng = np.random.RandomState(7)
    src = rng.randint(2, 60, size=(rows, 6)).astype(np.int32)
    tgt = rng.randint(2, 60, size=(rows, 6)).astype(np.int32)
    return src, tgt, rng.randint(0, 2, rows).astype(np.float32)


def _row_values(p, cfg, src, tgt, labels):
    """float32 row losses / accuracies from the oracle (what the device's rows are), summed in float64 by the caller."""
    from oracle import sse_oracle as O
    labels = np.asarray(labels, np.float32)
    if len(labels) == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    ns, nt = O.encode(p, cfg, "src", src), O.encode(p, cfg, "tgt", tgt)
    x = O.LOGIT_SCALE * np.sum(ns * nt, axis=-1, dtype=np.float32)
    s = O.sigmoid(x)
    acc = labels * np.floor(s + np.float32(0.1)) + (np.float32(1.0) - labels) * np.floor(np.float32(1.1) - s)
    return O.weighted_cross_entropy_with_logits(labels, x, 1.0), acc.astype(np.float32)


class EvalEngine(object):
    """eval_loss_sums / eval_loss_rows_sums from the oracle, plus the two calls DataParallelTrainer's constructor makes."""

    def __init__(self, p, cfg, corpora=None):
        self.p, self.cfg, self.corpora = p, cfg, corpora

    def train_grad_count(self):
        return 4

    def train_bind_arena(self, tensor):
        pass

    def eval_loss_sums(self, src, tgt, labels):
        per, acc = _row_values(self.p, self.cfg, src, tgt, labels)
        return float(per.sum(dtype=np.float64)), float(acc.sum(dtype=np.float64)), float(len(labels))

    def eval_loss_rows_sums(self, src_rows, tgt_rows, labels):
        return self.eval_loss_sums(self.corpora[0][src_rows], self.corpora[1][tgt_rows], labels)


def _dp_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["SSE_NO_TORCH"] = "1"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sse_amd
    from oracle import sse_oracle as O
    cfg = _dp_cfg()
    src, tgt, z = _dp_batch(23)
    tr = sse_amd.DataParallelTrainer(EvalEngine(O.init_params(cfg, seed=3), cfg, corpora=(src, tgt)))
    res = []
    for cut in (16, 23, 0):                                        # uneven shares; a rank with no row at all
        sl = slice(0, cut) if rank == 0 else slice(cut, 23)
        res.append(tr.eval_loss(src[sl], tgt[sl], z[sl]))
        rows = np.arange(23, dtype=np.int32)[sl]
        res.append(tr.eval_loss(rows, rows, z[sl], by_rows=True))
    np.save(os.path.join(out_dir, "ev%d.npy" % rank), np.array(res, np.float64))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_eval_loss_is_the_loss_of_the_whole_batch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import sse_oracle as O
    world, port = 2, free_port()
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    cfg = _dp_cfg()
    p = O.init_params(cfg, seed=3)
    src, tgt, z = _dp_batch(23)
    per, acc = _row_values(p, cfg, src, tgt, z)
    want = np.array([per.sum(dtype=np.float64) / 23, acc.sum(dtype=np.float64) / 23])
    assert 0.0 < want[1] < 1.0
    r0, r1 = (np.load(os.path.join(str(tmp_path), "ev%d.npy" % r)) for r in range(2))
    assert r0.shape == (6, 2) and np.array_equal(r0, r1)              # every rank holds the global numbers
    assert (np.abs(r0 - want) <= 1e-12 * np.abs(want)).all(), (r0, want)   # double sums of the same fp32 rows, another order
    # ... and they are the oracle's loss / acc of the undivided batch
    loss, acc_all, _ = O.loss_and_acc(O.encode(p, cfg, "src", src), O.encode(p, cfg, "tgt", tgt), z)
    assert abs(want[0] - float(loss)) <= 1e-6 * float(loss) and abs(want[1] - float(acc_all)) <= 1e-6
