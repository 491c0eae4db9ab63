"""One rank of tests/test_gpu_confusions_two_ranks.py: `python confusions_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peers, all on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows of the index only, runs ShardedIndex.score_confusions with the job's GLOBAL
positives once per margin of the job and writes rank<RANK>.npz.  It asserts nothing about numbers: the parent does."""
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
    pos = torch.from_numpy(z["pos"]).cuda()
    k = int(job["k"])
    res = {}
    for i, margin in enumerate(job["margins"]):
        out = sh.score_confusions(qd, k, pos, float(margin))
        for name, a in zip(("scores", "ids", "counts", "pos_scores", "pos_ids"), out):
            res["%s%d" % (name, i)] = a.cpu().numpy()
    for label, kw in (("bad_k", dict(k=1025)), ("bad_margin", dict(margin=float("nan")))):
        res[label] = RW.error_text(lambda: sh.score_confusions(qd, kw.get("k", k), pos, kw.get("margin", 0.0)))
    res["bruteforce"] = np.array(h.get_counter("score_confusions_bruteforce_queries"))
    RW.finish(job, rank, res, h)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
