"""One rank of tests/test_gpu_after_two_ranks.py: `python after_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peers, all on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows and tag words of the index only, runs ShardedIndex.score_topk_after with the
job's global cursors, then once more with the cursors its own first page ends on, and writes rank<RANK>.npz.  It asserts
nothing about numbers: the parent does."""
import datetime
import json
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
    with open(job_path) as f:
        job = json.load(f)
    z = np.load(job["inputs"])
    import torch
    import torch.distributed as dist
    import sse_amd
    from tests.util import make_pair, model_params
    world = job["world"]
    torch.cuda.set_device(0)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(job["port"]))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    t, q = z["t"], z["q"]
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 8, 4))
    h = m.handle
    sh = sse_amd.ShardedIndex(h, rank, world, t.shape[0])
    assert (sh.start, sh.end) == tuple(job["bounds"][rank])
    sh.set_local_rows(torch.from_numpy(t[sh.start:sh.end].copy()).cuda())
    sh.set_local_tags(torch.from_numpy(z["tags"][sh.start:sh.end].copy().view(np.int64)).cuda())
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
    try:
        sh.score_topk_after(qd, 1025)
        res["bad_k"] = np.array("no error")
    except ValueError as e:
        res["bad_k"] = np.array("ValueError: %s" % e)
    res["bruteforce"] = np.array(h.get_counter("score_after_bruteforce_queries"))
    torch.cuda.synchronize()
    h.close()
    np.savez(os.path.join(job["out_dir"], "rank%d.npz" % rank), **res)
    print("rank %d done" % rank, flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
