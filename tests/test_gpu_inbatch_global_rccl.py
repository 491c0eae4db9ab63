"""DataParallelTrainer(global_negatives=True, always_reduce=True) in a 1-rank `nccl` group on the one GPU of a test box: the
all-gather of the exchange block and the arena's all-reduce run through RCCL on buffers the library writes through raw
pointers, ordered by the stream the trainer hands over.  At world = 1 the global batch is the rank's own, so the step must equal
the handle's own train_loss = 1 step: the same loss and accuracy bits, every variable whose gradient is reduced in a fixed order
bit for bit (tests/test_gpu_train_state.py: all but the atomically scattered lookup tables), those within util.GRAD_BARS_EXACT."""
import os
import socket

import numpy as np
import pytest

from tests import inbatch_cases as IC
from tests.test_gpu_train_state import ATOMIC
from tests.util import GRAD_BARS_EXACT, LOSS_REL_EXACT, check_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nccl_group():
    import torch
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


@pytest.mark.parametrize("cid,even", [("dual-unpaired-b40", False), ("seo-b40", True)])
def test_one_rank_group_equals_the_handles_own_inbatch_step(nccl_group, cid, even):
    """even: rows_global is passed and the row counts come from shard_bounds instead of the tiny all-gather."""
    import sse_amd
    c = IC.STEP_CASES_BY_ID[cid]
    params, p = IC.step_params(c)
    src, tgt, z = IC.step_batch(c)
    models = []
    for _ in range(2):
        m = sse_amd.SSEModel(params)
        m.set_variables(p)
        m.handle.set_option("train_pair_dedup", 0)
        models.append(m)
    ref, m = models
    ref.handle.set_option("train_loss", 1)
    ref.handle.set_option("train_loss_scale", c["scale"])
    tr = sse_amd.DataParallelTrainer(m.handle, device="cuda:0", always_reduce=True, sparse_embedding=False, global_negatives=True,
                                     options={"train_loss_scale": c["scale"]})
    want = ref.train_step(src, tgt, z)
    got = tr.train_step(src, tgt, z, rows_global=len(z) if even else None)
    assert got == want, (got, want)
    assert tr.last_exchange == "dense"
    assert m.handle.get_counter("train_global_inbatch_steps") == 1 and m.handle.get_counter("train_inbatch_steps") == 0
    a, b = m.get_variables(with_slots=True), ref.get_variables(with_slots=True)
    for n in a:
        if n.split("/Adagrad")[0] not in ATOMIC:
            assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n
    check_grads({n: a[n] for n in a}, {n: b[n].astype(np.float64) for n in b}, GRAD_BARS_EXACT, what="variables after the step: ")
    # a second step on the same buffers (the atomically scattered tables differ in their last bits by now: no bit claim)
    want = ref.train_step(src, tgt, z)
    got = tr.train_step(src, tgt, z, rows_global=len(z) if even else None)
    assert abs(got[0] - want[0]) <= LOSS_REL_EXACT * abs(want[0]) + 1e-7 and abs(got[1] - want[1]) <= 1e-6, (got, want)
    m.handle.set_stream(0)
