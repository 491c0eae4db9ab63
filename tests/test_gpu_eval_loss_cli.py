"""sse_train --eval_loss on the GPU: a short run on the rawdata-qna fixture logs the held-out pair loss after the epoch's
task evaluation; without the flag the log has no such line."""
import logging
import math
import os
import re

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_QNA = os.path.join(ROOT, "tests", "golden", "rawdata-qna")
HELD_OUT = re.compile(r"held-out pair loss: (\S+), binary acc: (\S+) \((\d+) pairs\)")


def _train(mdir, *extra):
    from sse_amd import sse_train
    try:
        sse_train.main(["--task_type=qna", "--data_dir=" + RAW_QNA, "--model_dir=" + mdir, "--max_epoc=1",
                        "--steps_per_checkpoint=2", "--batch_size=8", "--network_mode=dual-encoder", "--src_cell_size=64",
                        "--tgt_cell_size=64", "--encoding_size=32", "--vocab_size=8000", "--max_seq_length=40", "--seed=0",
                        "--max_steps=3"] + list(extra))
    finally:
        for hd in logging.getLogger("").handlers:
            hd.close()
        logging.getLogger("").handlers.clear()
    return open(os.path.join(mdir, "TrainingLog.txt")).read()


def test_sse_train_logs_the_held_out_pair_loss_only_when_asked(tmp_path):
    from sse_amd import sse_data
    mdir = str(tmp_path / "models-qna")
    first = _train(mdir)                                            # default flag: the log as it always was
    assert "top 1/3/10 accuracies" in first and not HELD_OUT.search(first) and "held-out" not in first
    log = _train(mdir, "--eval_loss=1")[len(first):]                # continues from the checkpoint of the first run
    assert "Reading model parameters" in log
    found = HELD_OUT.findall(log)
    assert len(found) == 1, log
    loss, acc, pairs = float(found[0][0]), float(found[0][1]), int(found[0][2])
    data = sse_data.Data(mdir, RAW_QNA, 8000, 40, log=lambda *a: None)
    assert pairs == 2 * len(data.rawEvalCorpus) and pairs > 0
    assert math.isfinite(loss) and loss > 0.0 and 0.0 <= acc <= 1.0
    assert log.index("top 1/3/10 accuracies") < log.index("held-out pair loss")   # after the epoch's task evaluation
