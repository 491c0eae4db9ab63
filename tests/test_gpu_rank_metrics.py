"""Evaluator.ranks / rank_metrics and `sse_train --eval_ranks 1` on the GPU: a small stand-in model with 571 targets and 700
evaluation sources (two batches of the reference's 600; a third of the sources carry two labels).  The ranks are judged on
identical inputs -- the GPU's own source encodings and the index file's float64 rows through the oracle's full sort --
and the saturating numbers must still be Evaluator.eval's, exactly."""
import logging
import os
import re

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import rank_cases as RC
from tests.util import make_pair, model_params, random_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_QNA = os.path.join(ROOT, "tests", "golden", "rawdata-qna")
N_TGT, N_SRC, T, S = 571, 700, 12, 64


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    """(evaluator, model, source ids, labels as row numbers): built once, shared, left unchanged"""
    import sse_amd
    from sse_amd import sse_evaluator
    m, _ = make_pair(model_params("dual-encoder", 200, 16, 32, 32, S, T))
    rng = np.random.RandomState(12)
    tgt = random_ids(rng, N_TGT, T, 200, pad_frac=0.5)
    src = random_ids(rng, N_SRC, T, 200, pad_frac=0.5)
    enc = m.handle.encode(1, tgt, True)
    path = str(tmp_path_factory.mktemp("rank_metrics") / "targetEncodingIndex.tsv")
    with open(path, "w", encoding="utf-8") as f:
        for i, row in enumerate(enc):
            f.write("t%d\ttarget %d\t%s\n" % (i, i, ",".join(repr(float(v)) for v in row)))
    labels = [sorted(rng.choice(N_TGT, size=2 if i % 3 == 0 else 1, replace=False).tolist()) for i in range(N_SRC)]
    corpus = [(src[i].tolist(), ["t%d" % j for j in labels[i]]) for i in range(N_SRC)]
    ev = sse_evaluator.Evaluator(m, corpus, path, sse_amd.Session(m))
    return ev, m, src, labels


def test_rank_metrics_against_the_oracle_on_the_gpus_own_encodings(standin):
    ev, m, src, labels = standin
    assert ev.eval_Labels == labels
    brute0 = m.handle.get_counter("score_rank_bruteforce_pairs")
    got = ev.ranks()
    gpu_src = m.handle.encode(0, src, True)
    scores = O.scores_f64(gpu_src, ev.targetEncodings)
    ssc, _ = O.sorted_results(scores)
    gap = float(np.min(ssc[:, :-1] - ssc[:, 1:]))
    assert gap > 1e-12, gap            # two float64 summation orders differ by < S 2^-53 = 7e-15 on unit vectors
    full = RC.ranks_from_scores(scores)
    want = [full[i, labels[i]] for i in range(N_SRC)]
    assert len(got) == N_SRC and all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got, want))
    assert m.handle.get_counter("score_rank_bruteforce_pairs") == brute0
    rm = ev.rank_metrics()
    best = np.array([w.min() for w in want])
    assert rm["mrr"] == float(np.mean(1.0 / (1.0 + best)))
    assert rm["mean_rank"] == float(np.mean(1.0 + best))
    assert rm["median_rank"] == float(np.median(1.0 + best))
    assert best.max() >= 10            # labels do fall out of the top 10 here: what eval() cannot see
    # the saturating numbers are the evaluator's own, exactly, and the oracle's restatement of them
    acc = ev.eval((1, 3, 10))
    assert rm["tight_acc"] == acc
    assert acc == pytest.approx(O.evaluator_accuracy(gpu_src, ev.targetEncodings, labels), abs=1e-12)
    assert ev.rank_metrics(top_n=(5,), batch=250)["tight_acc"] == ev.eval((5,), batch=250)


def test_ranks_reupload_the_index_after_it_was_replaced(standin):
    ev, m, src, labels = standin
    want = ev.ranks()
    m.handle.index_upload(np.eye(4, S, dtype=np.float32))       # somebody else's index on the shared handle
    got = ev.ranks()
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


RANK_LINE = re.compile(r"label ranks over the whole index: MRR (\S+), mean rank (\S+), median rank (\S+) \((\d+) sources\)")


def test_sse_train_logs_the_rank_line_when_asked(tmp_path):
    from sse_amd import sse_data, sse_train
    mdir = str(tmp_path / "models-qna")
    try:
        sse_train.main(["--task_type=qna", "--data_dir=" + RAW_QNA, "--model_dir=" + mdir, "--max_epoc=1",
                        "--steps_per_checkpoint=2", "--batch_size=8", "--network_mode=dual-encoder", "--src_cell_size=64",
                        "--tgt_cell_size=64", "--encoding_size=32", "--vocab_size=8000", "--max_seq_length=40", "--seed=0",
                        "--max_steps=3", "--eval_ranks=1"])
    finally:
        for hd in logging.getLogger("").handlers:
            hd.close()
        logging.getLogger("").handlers.clear()
    log = open(os.path.join(mdir, "TrainingLog.txt")).read()
    found = RANK_LINE.findall(log)
    assert len(found) == 1, log
    mrr, mean_rank, median_rank, sources = float(found[0][0]), float(found[0][1]), float(found[0][2]), int(found[0][3])
    data = sse_data.Data(mdir, RAW_QNA, 8000, 40, log=lambda *a: None)
    assert sources == len(data.rawEvalCorpus) and sources > 0
    assert 0.0 < mrr <= 1.0 and 1.0 <= median_rank and 1.0 <= mean_rank and 1.0 / mean_rank <= mrr + 1e-6
    assert log.index("top 1/3/10 accuracies") < log.index("label ranks over the whole index")
