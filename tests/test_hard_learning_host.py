"""Host side of hard learning, no GPU: Data.get_hard_learning_train_batch[_rows] on the rawdata-qna fixture with a hand-made
confusion table, and compute_training_confusion_samples' bookkeeping (sources over 64 positives, the reference's spelling) with
a stand-in model whose handle answers from numpy."""
import os

import numpy as np
import pytest

import sse_amd  # noqa: F401
from sse_amd import sse_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_QNA = os.path.join(ROOT, "tests", "golden", "rawdata-qna")
T, N_CONF = 40, 4


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("hard"))
    sse_data.Data(d, RAW_QNA, 8000, T, seed=0, log=lambda *a: None)      # builds the cache once
    return d


def _data(work, seed):
    return sse_data.Data(work, RAW_QNA, 8000, T, seed=seed, log=lambda *a: None)


def _with_table(data, seed=5):
    """a hand-made table: every third source has none; the others 1 .. N_CONF targets that are not their positives"""
    rng = np.random.RandomState(seed)
    n, N = len(data.rawTrainPosCorpus), data.rawnegSetLen
    pad = data._positives_csr()[3]
    table = np.full((n, N_CONF), -1, np.int32)
    counts = np.zeros(n, np.int32)
    for i in range(n):
        if i % 3 == 0:
            continue
        c = 1 + i % N_CONF
        free = np.setdiff1d(np.arange(N), pad[i])
        table[i, :c] = rng.choice(free, size=c, replace=False)
        counts[i] = c
    data.confusions, data.confusion_counts = table, counts
    return data


class _NoRead(object):
    def __getitem__(self, i):
        raise AssertionError("the table was read")


def test_no_table_is_a_runtime_error_naming_the_call(work):
    d = _data(work, 0)
    for call in (lambda: d.get_hard_learning_train_batch_rows(8), lambda: d.get_hard_learning_train_batch(8)):
        with pytest.raises(RuntimeError, match="compute_training_confusion_samples"):
            call()


def test_negatives_come_from_the_table_row_and_are_never_positives(work):
    d = _with_table(_data(work, 1))
    pad = d._positives_csr()[3]
    seen_hard = seen_uniform = 0
    for _ in range(40):
        src, tgt, lab = d.get_hard_learning_train_batch_rows(16, hard_fraction=1.0)
        assert src.dtype == np.int32 and tgt.dtype == np.int32 and lab.dtype == np.float32
        assert np.array_equal(src[0::2], src[1::2]) and np.array_equal(lab, np.tile(np.array([1.0, 0.0], np.float32), len(src) // 2))
        assert (np.diff(src[0::2]) == 1).all() and len(src) <= 32          # one window, each source twice
        for i, p, ng in zip(src[0::2], tgt[0::2], tgt[1::2]):
            assert p in pad[i] and ng not in pad[i] and 0 <= ng < d.rawnegSetLen
            if d.confusion_counts[i] > 0:
                assert ng in d.confusions[i, :d.confusion_counts[i]]
                seen_hard += 1
            else:
                seen_uniform += 1
    assert seen_hard > 100 and seen_uniform > 50


def test_every_table_entry_of_a_source_is_drawn(work):
    d = _with_table(_data(work, 2))
    got = {}
    for _ in range(300):
        src, tgt, _ = d.get_hard_learning_train_batch_rows(16)
        for i, ng in zip(src[1::2], tgt[1::2]):
            got.setdefault(int(i), set()).add(int(ng))
    full = [i for i, s in got.items() if d.confusion_counts[i] == N_CONF and s == set(d.confusions[i].tolist())]
    assert len(full) > 10


def test_hard_fraction_zero_never_reads_the_table_and_is_the_plain_batch(work):
    d = _data(work, 3)
    d.confusions, d.confusion_counts = _NoRead(), _NoRead()
    plain = _data(work, 3)
    for _ in range(5):
        a = d.get_hard_learning_train_batch_rows(8, hard_fraction=0.0)
        b = plain.get_train_batch_rows(8)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_fraction_between_mixes_both(work):
    d = _with_table(_data(work, 4))
    hard = total = 0
    for _ in range(200):
        src, tgt, _ = d.get_hard_learning_train_batch_rows(16, hard_fraction=0.5)
        for i, ng in zip(src[1::2], tgt[1::2]):
            if d.confusion_counts[i] > 0:
                total += 1
                hard += int(ng in d.confusions[i, :d.confusion_counts[i]])
    # a uniform draw lands in a table row of at most 4 of 571 targets with probability < 1 %: the share is 0.5 within 5 sigma
    assert total > 1000 and abs(hard / total - 0.5) < 5 * 0.5 / np.sqrt(total) + 0.01


@pytest.mark.parametrize("target_rows", [False, True])
def test_list_form_and_rows_form_agree_for_the_same_seed(work, target_rows):
    a, b = _with_table(_data(work, 6)), _with_table(_data(work, 6))
    for _ in range(3):
        src_rows, tgt_rows, lab_rows = a.get_hard_learning_train_batch_rows(8, 0.7)
        src, tgt, lab = b.get_hard_learning_train_batch(8, target_rows=target_rows, hard_fraction=0.7)
        assert isinstance(src, list) and lab == [1.0, 0.0] * (len(src) // 2) and np.array_equal(lab_rows, lab)
        assert src == [b.rawTrainPosCorpus[r][0] for r in src_rows]
        if target_rows:
            assert tgt == [int(r) for r in tgt_rows]
        else:
            assert tgt == [b.encodedFullTargetSpace[b.fullSetTargetIds[r]] for r in tgt_rows]


class _Handle(object):
    """score_confusions from numpy on unit one-hot encodings"""

    def index_upload(self, rows):
        self.index = np.asarray(rows, np.float64)

    def score_confusions(self, q, k, pos, margin):
        assert pos.shape[1] <= 64 and pos.dtype == np.int64
        s = np.asarray(q, np.float64) @ self.index.T
        Q, N = s.shape
        sc, ids, cnt = np.full((Q, k), -np.inf), np.full((Q, k), np.iinfo(np.int64).max, np.int64), np.zeros(Q, np.int32)
        pm, pb = np.full(Q, -np.inf), np.full(Q, np.iinfo(np.int64).max, np.int64)
        for qi in range(Q):
            rows = np.unique(pos[qi][pos[qi] >= 0])
            j = np.lexsort((rows, -s[qi, rows]))[0]
            pm[qi], pb[qi] = s[qi, rows[j]], rows[j]
            ok = np.ones(N, bool)
            ok[rows] = False
            cols = np.flatnonzero(ok & (s[qi] >= pm[qi] - margin))
            o = cols[np.lexsort((cols, -s[qi, cols]))][:k]
            sc[qi, :len(o)], ids[qi, :len(o)], cnt[qi] = s[qi, o], o, len(o)
        return sc, ids, cnt, pm, pb


class _Model(object):
    network_mode = "dual-encoder"

    def __init__(self, data, S=16):
        rng = np.random.RandomState(9)
        self.targetSpaceSize = data.rawnegSetLen
        self.w = rng.standard_normal((T, S))
        self.handle = _Handle()

    def _enc(self, ids):
        x = np.tanh(np.asarray(ids, np.float64) / 4000.0 @ self.w) + 1e-3
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)

    encode_source = encode_target = lambda self, ids, normalize=True: self._enc(ids)


def test_compute_keeps_table_counts_and_stats_and_skips_sources_over_64(work):
    d = _data(work, 7)
    assert sse_data.Data.compute_training_confusion_sampes is sse_data.Data.compute_training_confusion_samples
    many = d.fullSetTargetIds[:65]
    d.rawTrainPosCorpus = list(d.rawTrainPosCorpus) + [(d.rawTrainPosCorpus[0][0], many)]      # a synthetic source with 65 targets
    n = len(d.rawTrainPosCorpus)
    model = _Model(d)
    st = d.compute_training_confusion_sampes(model, n=3, margin=0.05, chunk=100)
    assert st is d.confusion_stats and st["sources"] == n and st["skipped_over_64"] == 1
    assert d.confusions.shape == (n, 3) and d.confusions.dtype == np.int32 and d.confusion_counts.dtype == np.int32
    assert d.confusion_counts[-1] == 0 and (d.confusions[-1] == -1).all()
    assert st["with_confusions"] == int((d.confusion_counts > 0).sum()) and abs(st["mean_count"] - d.confusion_counts.mean()) < 1e-12
    # against the stand-in handle asked source by source
    src, tgt = d.corpus_matrices()
    pad = d._positives_csr()[3]
    model.handle.index_upload(model.encode_target(tgt))
    top1 = 0
    for i in range(n - 1):
        sc, ids, cnt, pm, _ = model.handle.score_confusions(model.encode_source(src[i:i + 1]), 3, pad[i:i + 1, :64], 0.05)
        assert d.confusion_counts[i] == cnt[0] and np.array_equal(d.confusions[i, :cnt[0]], ids[0, :cnt[0]])
        assert (d.confusions[i, cnt[0]:] == -1).all()
        top1 += int(not (sc[0, :cnt[0]] >= pm[0]).any())
    assert abs(st["train_top1"] - top1 / float(n - 1)) < 1e-12 and 0 < st["with_confusions"] < n
    # and the batches draw from it
    s_rows, t_rows, _ = d.get_hard_learning_train_batch_rows(8)
    for i, ng in zip(s_rows[1::2], t_rows[1::2]):
        if d.confusion_counts[i] > 0:
            assert ng in d.confusions[i, :d.confusion_counts[i]]
