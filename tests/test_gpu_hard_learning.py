"""Hard learning on the GPU: Data.compute_training_confusion_samples on the rawdata-qna fixture (602 sources, 93 targets) with a
tiny dual-encoder and a source-encoder-only model, held to the numpy reference of tests/confusion_cases.py fed with the DEVICE'S
OWN encodings -- so the encoder's error cannot move a row across the floor; a source whose reference is not decidable to within
two float64 summation orders (CC.rows_decidable) is left out, and at most 2 % may be.  (With the float64 oracle's encodings of
the same weights, seed 0, no source of either model is left out: checked on the CPU when the seed was fixed.)  Then sse_train:
--hard_learning 4 logs the `hard learning:` line every epoch and finishes on both batch paths, and --hard_learning 0 with the
other hard_* flags set leaves every log line as it is without any of them."""
import logging
import os
import re

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import confusion_cases as CC
from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_QNA = os.path.join(ROOT, "tests", "golden", "rawdata-qna")
T, S, N_CONF, MARGIN = 40, 16, 4, 0.01     # (untrained weights: at 0.1 the floor of the dual-encoder cuts no list of 4)
HARD_LINE = re.compile(r"hard learning: (\d+) of (\d+) sources have confusions \(mean (\S+) per source\), training top-1 (\S+)")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from sse_amd import sse_data
    return sse_data.Data(str(tmp_path_factory.mktemp("hard")), RAW_QNA, 8000, T, seed=0, log=lambda *a: None)


@pytest.mark.parametrize("mode", ["dual-encoder", "source-encoder-only"])
def test_confusion_table_is_the_reference_on_the_devices_own_encodings(data, mode):
    src, tgt = data.corpus_matrices()
    n, N = src.shape[0], tgt.shape[0]
    m, _ = make_pair(model_params(mode, data.vocab_size, 8, 16, 16, S, T, N=N))
    m.set_forward_only(True)
    st = data.compute_training_confusion_samples(m, n=N_CONF, margin=MARGIN)
    table, counts = data.confusions.copy(), data.confusion_counts.copy()
    assert table.shape == (n, N_CONF) and table.dtype == np.int32 and counts.dtype == np.int32 and st["skipped_over_64"] == 0
    # the same encodings once more: what the table was computed from, bit for bit
    index = m.encode_target(np.zeros((N, T), np.int32) if mode == "source-encoder-only" else tgt, True)
    q = m.encode_source(src, True)
    pad = data._positives_csr()[3]
    again = m.handle.score_confusions(q, N_CONF, pad, MARGIN)
    live = np.arange(N_CONF)[None, :] < again[2][:, None]
    assert np.array_equal(np.where(live, again[1], -1), table) and np.array_equal(again[2], counts)
    m.handle.close()
    uniq, same = np.unique(index, axis=0, return_inverse=True)
    s = O.scores_f64(q, uniq.astype(np.float64))[:, same.reshape(-1)]     # bit-equal rows: one reference score
    qn = float(np.linalg.norm(q.astype(np.float64), axis=1).max())
    tn = float(np.linalg.norm(index.astype(np.float64), axis=1).max())
    bar = max(1e-12, 2.0 * S * 2.0 ** -53) * qn * tn
    good = CC.rows_decidable(s, pad, MARGIN, N_CONF, bar, same.reshape(-1))
    left_out = int((~good).sum())
    ws, wi, wc, wm, wb = CC.reference_arrays(s, pad, MARGIN, N_CONF)
    print("HARDL %s: %d sources, %d left out, %d with confusions, mean %.3f, top-1 %.4f, worst |pos score - oracle| %.3e (bar %.3e)"
          % (mode, n, left_out, st["with_confusions"], st["mean_count"], st["train_top1"], np.abs(again[3] - wm).max(), bar))
    assert left_out <= 0.02 * n
    want = np.where(np.arange(N_CONF)[None, :] < wc[:, None], wi, -1).astype(np.int32)
    assert np.array_equal(table[good], want[good]) and np.array_equal(counts[good], wc[good])
    assert np.array_equal(again[4], wb) and np.abs(again[3] - wm).max() <= bar
    assert st["sources"] == n and st["with_confusions"] == int((counts > 0).sum()) and abs(st["mean_count"] - counts.mean()) < 1e-12
    top1 = np.array([not (ws[i, :wc[i]] >= wm[i]).any() for i in range(n)])
    assert abs(st["train_top1"] - top1.mean()) <= left_out / float(n) + 1e-12
    assert 0 < st["with_confusions"] and (counts < N_CONF).any()          # the floor cuts some lists and leaves others


def _train(mdir, *extra):
    from sse_amd import sse_train
    try:
        sse_train.main(["--task_type=qna", "--data_dir=" + RAW_QNA, "--model_dir=" + mdir, "--max_epoc=2",
                        "--steps_per_checkpoint=2", "--batch_size=8", "--network_mode=dual-encoder", "--src_cell_size=32",
                        "--tgt_cell_size=32", "--encoding_size=16", "--vocab_size=8000", "--max_seq_length=40", "--seed=0"]
                       + list(extra))
    finally:
        for hd in logging.getLogger("").handlers:
            hd.close()
        logging.getLogger("").handlers.clear()
    return open(os.path.join(mdir, "TrainingLog.txt")).read()


def _lines(log, mdir):
    """the log's messages without what differs between two runs of the same thing: time stamps, wall times, the directory"""
    out = []
    for line in log.replace(mdir, "MDIR").splitlines():
        line = re.sub(r"^\d\d/\d\d/\d{4} \d\d:\d\d:\d\d [AP]M - ", "", line)
        line = re.sub(r"step-time:\S+", "step-time:X", line)
        out.append(re.sub(r"took \S+ hours", "took X hours", line))
    return out


def test_sse_train_hard_learning_runs_and_the_default_is_unchanged(tmp_path):
    a, b, c, d = (str(tmp_path / x) for x in ("plain", "off", "hard", "hard_lists"))
    plain = _train(a, "--max_steps=6")
    off = _train(b, "--max_steps=6", "--hard_learning=0", "--hard_margin=0.3", "--hard_fraction=0.9", "--hard_start_epoch=0")
    assert "hard learning" not in plain and _lines(plain, a) == _lines(off, b)
    assert "top 1/3/10 accuracies" in plain
    for mdir, extra in ((c, ()), (d, ("--device_corpus=0",))):
        log = _train(mdir, "--max_steps=6", "--hard_learning=4", "--hard_start_epoch=0", *extra)
        found = HARD_LINE.findall(log)
        assert len(found) == 1, log                                       # max_steps ends the run inside epoch 0
        have, total, mean, top1 = int(found[0][0]), int(found[0][1]), float(found[0][2]), float(found[0][3])
        assert total == 602 and 0 <= have <= total and 0.0 <= mean <= 4.0 and 0.0 <= top1 <= 1.0
        assert log.index("hard learning:") < log.index("top 1/3/10 accuracies") and any("ckpt-epoch-0" in f for f in os.listdir(mdir))
    # --hard_start_epoch: epoch 0 without the table, epoch 1 with it
    e = str(tmp_path / "late")
    log = _train(e, "--max_steps=76", "--steps_per_checkpoint=50", "--hard_learning=2", "--hard_start_epoch=1")
    assert len(HARD_LINE.findall(log)) == 1 and log.index("epoch# 0") < log.index("hard learning:") < log.index("epoch# 1")
