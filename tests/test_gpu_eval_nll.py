"""Evaluator.softmax_nll and `sse_train --eval_nll 1` on the GPU: the stand-in model of tests/test_gpu_rank_metrics.py (571
targets, 700 evaluation sources, a third of them with two labels).  The held-out full-softmax NLL is judged on identical inputs
-- the GPU's own source encodings and the index file's float64 rows, reduced in float64 by numpy -- within the summed bounds
the library certifies; the training command logs one finite nll line per epoch when asked and its old log otherwise."""
import logging
import math
import os
import re

import numpy as np
import pytest

from tests.util import make_pair, model_params, random_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_QNA = os.path.join(ROOT, "tests", "golden", "rawdata-qna")
N_TGT, N_SRC, T, S = 571, 700, 12, 64


def test_softmax_nll_against_float64_on_the_gpus_own_encodings(tmp_path):
    import sse_amd
    from sse_amd import sse_evaluator
    m, _ = make_pair(model_params("dual-encoder", 200, 16, 32, 32, S, T))
    rng = np.random.RandomState(12)
    tgt = random_ids(rng, N_TGT, T, 200, pad_frac=0.5)
    src = random_ids(rng, N_SRC, T, 200, pad_frac=0.5)
    enc = m.handle.encode(1, tgt, True)
    path = str(tmp_path / "targetEncodingIndex.tsv")
    with open(path, "w", encoding="utf-8") as f:
        for i, row in enumerate(enc):
            f.write("t%d\ttarget %d\t%s\n" % (i, i, ",".join(repr(float(v)) for v in row)))
    labels = [sorted(rng.choice(N_TGT, size=2 if i % 3 == 0 else 1, replace=False).tolist()) for i in range(N_SRC)]
    labels[5] = [labels[5][0], labels[5][0]]                     # a label named twice counts once
    corpus = [(src[i].tolist(), ["t%d" % j for j in labels[i]]) for i in range(N_SRC)]
    ev = sse_evaluator.Evaluator(m, corpus, path, sse_amd.Session(m))
    for scale in (64.0, 16.0):
        calls0 = m.handle.get_counter("score_lse_calls")
        got = ev.softmax_nll(scale=scale)
        assert m.handle.get_counter("score_lse_calls") == calls0 + 1          # one chunk: one call
        lse, bound, scores = ev.softmax_terms(scale)
        gpu_src = m.handle.encode(0, src, True)
        z = scale * (gpu_src.astype(np.float64) @ ev.targetEncodings.T)       # float64 rows of the index file
        want_lse = np.logaddexp.reduce(z, axis=1)
        assert (np.abs(lse - want_lse) <= bound).all() and bound.max() < 1e-2
        nll = np.array([want_lse[i] - np.logaddexp.reduce(z[i, sorted(set(labels[i]))]) for i in range(N_SRC)])
        # the label term comes from score_rank's float64 scores: another summation order, S 2^-53 per unit-vector dot product
        slack = float(bound.sum()) / N_SRC + scale * 4 * S * 2.0 ** -53
        assert abs(got["nll"] - float(nll.mean())) <= slack, (got, float(nll.mean()), slack)
        assert abs(got["label_prob"] - float(np.exp(-nll).mean())) <= slack
        assert (nll > 0).all() and 0.0 < got["label_prob"] < 1.0
        assert len(scores[5]) == 1 and len(scores[0]) == 2
        print("NLL scale %g: nll %.6f (float64 %.6f, slack %.3e), label prob %.6f" % (scale, got["nll"], nll.mean(), slack, got["label_prob"]))
    # the index is put back after somebody replaced it
    m.handle.index_upload(np.eye(4, S, dtype=np.float32))
    assert ev.softmax_nll(scale=16.0) == got
    m.handle.close()


NLL_LINE = re.compile(r"held-out full-softmax nll over the whole index: (\S+), label prob: (\S+) \(scale (\d+), (\d+) sources\)")


def _train(mdir, *extra):
    from sse_amd import sse_train
    try:
        sse_train.main(["--task_type=qna", "--data_dir=" + RAW_QNA, "--model_dir=" + mdir, "--steps_per_checkpoint=2",
                        "--batch_size=8", "--network_mode=dual-encoder", "--src_cell_size=64", "--tgt_cell_size=64",
                        "--encoding_size=32", "--vocab_size=8000", "--max_seq_length=40", "--seed=0"] + list(extra))
    finally:
        for hd in logging.getLogger("").handlers:
            hd.close()
        logging.getLogger("").handlers.clear()
    return open(os.path.join(mdir, "TrainingLog.txt")).read()


def _shape(log):
    """the log as line patterns: the message of every line with its numbers masked (no timestamps, no timings)"""
    out = []
    for line in log.splitlines():
        msg = line.split(" - ", 3)[-1]
        out.append(re.sub(r"[-+]?\d[\d.e+-]*", "#", msg))
    return out


def test_sse_train_logs_one_nll_line_per_epoch_only_when_asked(tmp_path):
    from sse_amd import sse_data
    pdir, mdir = str(tmp_path / "plain"), str(tmp_path / "flagged")
    plain = _train(pdir, "--max_epoc=1", "--max_steps=3")
    assert "top 1/3/10 accuracies" in plain and not NLL_LINE.search(plain) and "nll" not in plain
    log = _train(mdir, "--max_epoc=1", "--max_steps=3", "--eval_nll=1")
    found = NLL_LINE.findall(log)
    assert len(found) == 1 == log.count("top 1/3/10 accuracies"), log       # one epoch, one evaluation, one line
    data = sse_data.Data(mdir, RAW_QNA, 8000, 40, log=lambda *a: None)
    nll, prob, scale, sources = found[0]
    assert math.isfinite(float(nll)) and float(nll) > 0.0 and 0.0 < float(prob) <= 1.0
    assert int(scale) == 64 and int(sources) == len(data.rawEvalCorpus) > 0  # the pair loss trains at 64
    assert log.index("top 1/3/10 accuracies") < log.index("held-out full-softmax nll")
    # with the nll line taken out, the log has the line patterns of the log without the flag
    assert [s for s in _shape(log.replace(mdir, "MDIR")) if "full-softmax nll" not in s] == _shape(plain.replace(pdir, "MDIR"))
    # under the in-batch loss the line carries the scale the run trains with
    inb = _train(str(tmp_path / "inbatch"), "--max_epoc=1", "--max_steps=3", "--loss=inbatch", "--loss_scale=32", "--eval_nll=1")
    assert [f[2] for f in NLL_LINE.findall(inb)] == ["32"]
