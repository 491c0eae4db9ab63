"""One rank of tests/test_gpu_confusions_two_ranks.py: `python confusions_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peers, all on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows of the index only, runs ShardedIndex.score_confusions with the job's GLOBAL
positives once per margin of the job and writes rank<RANK>.npz.  It asserts nothing about numbers: the parent does."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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
    qd = torch.from_numpy(q).cuda()
    pos = torch.from_numpy(z["pos"]).cuda()
    k = int(job["k"])
    res = {}
    for i, margin in enumerate(job["margins"]):
        out = sh.score_confusions(qd, k, pos, float(margin))
        for name, a in zip(("scores", "ids", "counts", "pos_scores", "pos_ids"), out):
            res["%s%d" % (name, i)] = a.cpu().numpy()
    for label, kw in (("bad_k", dict(k=1025)), ("bad_margin", dict(margin=float("nan")))):
        try:
            sh.score_confusions(qd, kw.get("k", k), pos, kw.get("margin", 0.0))
            res[label] = np.array("no error")
        except ValueError as e:
            res[label] = np.array("ValueError: %s" % e)
    res["bruteforce"] = np.array(h.get_counter("score_confusions_bruteforce_queries"))
    torch.cuda.synchronize()
    h.close()
    np.savez(os.path.join(job["out_dir"], "rank%d.npz" % rank), **res)
    print("rank %d done" % rank, flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
