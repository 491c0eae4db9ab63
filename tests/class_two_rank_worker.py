"""One rank of tests/test_gpu_class_two_ranks.py: `python class_two_rank_worker.py JOB.json RANK`.

A fresh process (the pytest process has initialised the GPU already) that joins a `gloo` group on 127.0.0.1 with its peer, both
on device 0, loads the job's weights, takes ONE step of its own rows through the product's DataParallelTrainer under the job's
options and writes rank<RANK>.npz: the variables and slots afterwards, the step's (loss, accuracy), the exchange it used and the
train_* counters.  It asserts nothing about numbers: the parent does."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(job_path, rank):
    import torch
    import sse_amd
    from tests import rank_worker as RW
    job, z = RW.open_job(job_path)
    RW.join_group(job, rank)
    m = sse_amd.SSEModel(job["params"])
    m.set_variables({k[2:]: z[k] for k in z.files if k.startswith("p/")})
    tr = sse_amd.DataParallelTrainer(m.handle, device="cuda:0", options=job["options"])
    key = "rank%d/" % rank
    loss, acc = tr.train_step(z[key + "src"], z[key + "tgt"], z[key + "z"])      # uneven rows: rows_global from the all-gather
    torch.cuda.synchronize()
    res = {"v/" + n: v for n, v in m.get_variables(with_slots=True).items()}
    res["hist"] = np.array([loss, acc], np.float64)
    res["exchange"] = np.array(tr.last_exchange)
    for n in ("train_class_steps", "train_inbatch_steps", "train_path_fused"):
        res["counter/" + n] = np.array(m.handle.get_counter(n))
    RW.finish(job, rank, res)
    m.handle.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
