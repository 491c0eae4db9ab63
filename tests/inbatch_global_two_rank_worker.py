"""One rank of tests/test_gpu_inbatch_global_two_ranks.py: `python inbatch_global_two_rank_worker.py JOB.json RANK`.

A fresh process (the pytest process has initialised the GPU already) that joins a `gloo` group on 127.0.0.1 with its peer, both
on device 0.  Three runs of its own rows through the product's DataParallelTrainer under the job's options, each on a new
handle with the job's weights: ONE step with global_negatives=True, ONE step with global_negatives=False, and job["steps"]
steps with global_negatives=True.  It writes rank<RANK>.npz: per run the variables and slots afterwards and the (loss,
accuracy) of every step, the exchange used and the train_* counters.  It asserts nothing about numbers: the parent does."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COUNTERS = ("train_open_steps", "train_global_inbatch_steps", "train_inbatch_steps", "train_path_fused", "train_paired_steps")


def main(job_path, rank):
    import torch
    import torch.distributed as dist
    import sse_amd
    from tests import rank_worker as RW
    job, z = RW.open_job(job_path)
    RW.join_group(job, rank)
    key = "rank%d/" % rank
    res = {}
    for run, global_negatives, steps in (("global", True, 1), ("local", False, 1), ("long", True, int(job["steps"]))):
        m = sse_amd.SSEModel(job["params"])
        m.set_variables({k[2:]: z[k] for k in z.files if k.startswith("p/")})
        tr = sse_amd.DataParallelTrainer(m.handle, device="cuda:0", options=job["options"], global_negatives=global_negatives)
        hist = [tr.train_step(z[key + "src"], z[key + "tgt"], z[key + "z"]) for _ in range(steps)]   # uneven rows: counts from the all-gather
        torch.cuda.synchronize()
        res.update({"%s/v/%s" % (run, n): v for n, v in m.get_variables(with_slots=True).items()})
        res[run + "/hist"] = np.array(hist, np.float64)
        res[run + "/exchange"] = np.array(tr.last_exchange)
        for n in COUNTERS:
            res["%s/counter/%s" % (run, n)] = np.array(m.handle.get_counter(n))
        dist.barrier()
        m.handle.close()
    RW.finish(job, rank, res)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
