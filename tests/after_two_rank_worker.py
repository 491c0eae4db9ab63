"""One rank of tests/test_gpu_after_two_ranks.py: `python after_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peers, all on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows and tag words of the index only, runs ShardedIndex.score_topk_after with the
job's global cursors, then once more with the cursors its own first page ends on, and writes rank<RANK>.npz.  It asserts
nothing about numbers: the parent does."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def next_cursors(cs, ci, scores, ids, counts):
    """every query's last real entry; a query without one keeps its cursor"""
    cs, ci = cs.copy(), ci.copy()
    rows = np.flatnonzero(counts > 0)
    cs[rows], ci[rows] = scores[rows, counts[rows] - 1], ids[rows, counts[rows] - 1]
    return cs, ci


def main(job_path, rank):
    import torch
    from tests import rank_worker as RW
    job, z = RW.open_job(job_path)
    RW.join_group(job, rank)
    h, sh = RW.sharded_index(job, z, rank)
    q = z["q"]
    qd = torch.from_numpy(q).cuda()
    any_of = torch.from_numpy(z["any"].view(np.int64).copy()).cuda()
    k = int(job["k"])
    res = {}
    cs, ci = z["cs"], z["ci"]
    for page in (1, 2):
        sc, ids, cnt = sh.score_topk_after(qd, k, after=(torch.from_numpy(cs).cuda(), torch.from_numpy(ci).cuda()), any_of=any_of)
        sc, ids, cnt = sc.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().numpy()
        res.update({"scores%d" % page: sc, "ids%d" % page: ids, "counts%d" % page: cnt})
        cs, ci = next_cursors(cs, ci, sc, ids, cnt)
    sc, ids, cnt = sh.score_topk_after(qd, k, any_of=any_of)     # no cursor at all
    res.update(scores0=sc.cpu().numpy(), ids0=ids.cpu().numpy(), counts0=cnt.cpu().numpy())
    res["bad_k"] = RW.error_text(lambda: sh.score_topk_after(qd, 1025))
    res["bruteforce"] = np.array(h.get_counter("score_after_bruteforce_queries"))
    RW.finish(job, rank, res, h)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
