"""One rank of tests/test_gpu_grouped_two_ranks.py: `python grouped_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peers, all on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows, group keys and tag words of the index only, runs ShardedIndex.score_topk_grouped and writes
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
    sh.set_local_groups(torch.from_numpy(z["groups"][sh.start:sh.end].copy()).cuda())
    qd = torch.from_numpy(q).cuda()
    any_of = torch.from_numpy(z["any"].view(np.int64).copy()).cuda()
    none_of = torch.from_numpy(z["none"].view(np.int64).copy()).cuda()
    sc, ids, grp, cnt = sh.score_topk_grouped(qd, int(job["k"]), any_of=any_of, none_of=none_of)
    res = {"scores": sc.cpu().numpy(), "ids": ids.cpu().numpy(), "groups": grp.cpu().numpy(), "counts": cnt.cpu().numpy()}
    res["bad_k"] = RW.error_text(lambda: sh.score_topk_grouped(qd, 1025))
    res["bruteforce"] = np.array(h.get_counter("score_grouped_bruteforce_queries"))
    RW.finish(job, rank, res, h)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
