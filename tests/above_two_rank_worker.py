"""One rank of tests/test_gpu_above_two_ranks.py: `python above_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peers, all on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows of the index only, runs ShardedIndex.score_above / count_above and writes
rank<RANK>.npz.  It asserts nothing about numbers: the parent does."""
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
    q = z["q"]
    qd = torch.from_numpy(q).cuda()
    pq, thr = torch.from_numpy(z["pair_q"]).cuda(), torch.from_numpy(z["pair_thr"]).cuda()
    off, ids, sc = sh.score_above(qd, pq, thr)
    res = {"offsets": off.cpu().numpy(), "ids": ids.cpu().numpy(), "scores": sc.cpu().numpy(),
           "counts": sh.count_above(qd, pq, thr).cpu().numpy()}
    res["bad_q"] = RW.error_text(lambda: sh.score_above(qd, pq + q.shape[0], thr))
    e_off, e_ids, e_sc = sh.score_above(qd, pq[:0], thr[:0])
    res["empty_offsets"], res["empty_n"] = e_off.cpu().numpy(), np.array(e_ids.numel() + e_sc.numel())
    res["bruteforce"] = np.array(h.get_counter("score_above_bruteforce_pairs"))
    RW.finish(job, rank, res, h)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
