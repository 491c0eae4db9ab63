"""The class softmax step as two REAL ranks: two processes on the one GPU of a test box, a `gloo` group between them (host-staged
collectives), DataParallelTrainer with options {"train_class_loss": 1} on 5 + 9 pair rows over 40 classes.  The softmax over
the class table decomposes over the rows of a batch (the rows of one source kept on one rank), so the variables after the step
must equal those of ONE handle stepping the concatenated 14 rows, up to summation order: util.GRAD_BARS_EXACT, on the variables
and on the update itself.  The dense table gradient crosses the wire inside the arena's one all-reduce and enters the global
norm after it.  (The same comparison under train_loss = 1 does not hold -- in-batch negatives are the rank's own rows -- and is
not made.)  One launch of tests/class_two_rank_worker.py per rank, each under its own time limit; a child that fails ends the
launch and the other child is killed; a child that died of a signal ends the pytest session -- nothing more starts on the GPU
after a fault."""
import os

import numpy as np
import pytest

from tests import class_loss_cases as CC
from tests.util import GRAD_BARS_EXACT, check_grads
from tests.rank_launch import free_port, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "class_two_rank_worker.py")


ROWS = (5, 9)


def test_two_uneven_ranks_equal_one_handle_on_the_concatenated_batch(tmp_path):
    import sse_amd
    tmp = str(tmp_path)
    c = CC.STEP_CASES_BY_ID["seo-fused-b6-n40"]
    params, p = CC.step_params(c)
    parts = [CC.step_batch(c, seed=20 + r, B=B) for r, B in enumerate(ROWS)]
    src, tgt, z = (np.concatenate([part[k] for part in parts]) for k in range(3))
    for a in parts[0][0]:                                        # the rows of one source stay on one rank
        assert not (parts[1][0] == a).all(axis=1).any()
    assert all(len(np.unique(part[0], axis=0)) < len(part[0]) and part[2].sum() >= 2 for part in parts)
    inputs = {"p/" + k: v for k, v in p.items()}
    for r, part in enumerate(parts):
        inputs.update({"rank%d/src" % r: part[0], "rank%d/tgt" % r: part[1], "rank%d/z" % r: part[2]})
    np.savez(os.path.join(tmp, "inputs.npz"), **inputs)
    job = dict(world=2, port=free_port(), inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp, params=params,
               options={"train_class_loss": 1, "train_loss_scale": 64})
    out = launch(WORKER, tmp, 2, job)
    # one handle, the 14 rows at once
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    m.handle.set_option("train_class_loss", 1)
    before = m.get_variables(with_slots=True)
    loss, acc = m.train_step(src, tgt, z)
    after = m.get_variables(with_slots=True)
    names = sorted(after)
    for r in range(2):
        assert int(out[r]["counter/train_class_steps"]) == 1 and int(out[r]["counter/train_inbatch_steps"]) == 0
        assert str(out[r]["exchange"]) == "dense"
        for n in names:                                          # the update is the same on every rank, bit for bit
            assert out[r]["v/" + n].tobytes() == out[0]["v/" + n].tobytes(), n
        assert abs(out[r]["hist"][0] - loss) <= CC.LOSS_REL_EXACT * abs(loss) + 1e-7 and abs(out[r]["hist"][1] - acc) <= 1e-6
    got = {n: out[0]["v/" + n] for n in names}
    errs = check_grads(got, {n: after[n].astype(np.float64) for n in names}, GRAD_BARS_EXACT, what="variables after the step: ")
    moved = {n: got[n].astype(np.float64) - before[n] for n in names}
    want = {n: after[n].astype(np.float64) - before[n] for n in names}
    assert all(np.abs(want[n]).max() > 0 for n in names)
    derrs = check_grads(moved, want, GRAD_BARS_EXACT, what="the update itself: ")
    print("CLASS TWO RANKS: variables norm %.2e element %.2e; update norm %.2e element %.2e"
          % (max(e[0] for e in errs.values()), max(e[1] for e in errs.values()), max(e[0] for e in derrs.values()),
             max(e[1] for e in derrs.values())))
