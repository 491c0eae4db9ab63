"""What every rank of the multi-rank GPU tests does around its own work (tests/*_two_rank_worker.py, started by
tests/rank_launch.py): a fresh process that reads its job, joins a `gloo` group on 127.0.0.1 with its peers, all of them on
device 0 (the collectives are staged through the host, sse_amd/collectives.py), and in the end writes rank<RANK>.npz.  A
worker asserts nothing about numbers: the parent does."""
import datetime
import json
import os

import numpy as np


def open_job(job_path):
    """(the job, its inputs.npz)"""
    with open(job_path) as f:
        job = json.load(f)
    return job, np.load(job["inputs"])


def join_group(job, rank):
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(job["port"]))
    dist.init_process_group("gloo", rank=rank, world_size=job["world"], timeout=datetime.timedelta(seconds=60))


def sharded_index(job, z, rank):
    """(handle, ShardedIndex) of this rank over the inputs' index z["t"]: its rows uploaded, and its tag words when the
    inputs hold any."""
    import torch
    import sse_amd
    from tests.util import make_pair, model_params
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    sh = sse_amd.ShardedIndex(m.handle, rank, job["world"], z["t"].shape[0])
    assert (sh.start, sh.end) == tuple(job["bounds"][rank])
    sh.set_local_rows(torch.from_numpy(z["t"][sh.start:sh.end].copy()).cuda())
    if "tags" in z.files:
        sh.set_local_tags(torch.from_numpy(z["tags"][sh.start:sh.end].copy().view(np.int64)).cuda())
    return m.handle, sh


def error_text(fn):
    """what the parent checks of a call that must be refused: "ValueError: ..." -- or "no error" """
    try:
        fn()
        return np.array("no error")
    except ValueError as e:
        return np.array("ValueError: %s" % e)


def finish(job, rank, res, handle=None):
    """The closing sequence: with a handle, synchronise and close it; write the results, say so, leave the group together."""
    import torch
    import torch.distributed as dist
    if handle is not None:
        torch.cuda.synchronize()
        handle.close()
    np.savez(os.path.join(job["out_dir"], "rank%d.npz" % rank), **res)
    print("rank %d done" % rank, flush=True)
    dist.barrier()
    dist.destroy_process_group()
