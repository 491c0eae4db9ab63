"""One rank of tests/test_gpu_rank_two_ranks.py: `python rank_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peer, both on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows of the index only, runs ShardedIndex.rank_of and writes rank<RANK>.npz.  It
asserts nothing about numbers: the parent does."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(job_path, rank):
    import torch
    from tests import rank_worker as RW
    job, z = RW.open_job(job_path)
    RW.join_group(job, rank)
    h, sh = RW.sharded_index(job, z, rank)
    t, q = z["t"], z["q"]
    qd = torch.from_numpy(q).cuda()
    pq, pi = torch.from_numpy(z["pair_q"]).cuda(), torch.from_numpy(z["pair_id"]).cuda()
    res = {"ranks": sh.rank_of(qd, pq, pi).cpu().numpy()}
    res["bad_id"] = RW.error_text(lambda: sh.rank_of(qd, pq, pi + t.shape[0]))
    res["empty"] = sh.rank_of(qd, pq[:0], pi[:0]).cpu().numpy()
    res["bruteforce"] = np.array(h.get_counter("score_rank_bruteforce_pairs"))
    RW.finish(job, rank, res, h)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
