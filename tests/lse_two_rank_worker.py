"""One rank of tests/test_gpu_lse_two_ranks.py: `python lse_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peer, both on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows, tag words and bias values of the index only, runs ShardedIndex.score_lse and
writes rank<RANK>.npz.  It asserts nothing about numbers: the parent does."""
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
    sh.set_local_tags(torch.from_numpy(z["tags"][sh.start:sh.end].copy().view(np.int64)).cuda())
    sh.set_local_bias(torch.from_numpy(z["bias"][sh.start:sh.end].copy()).cuda())
    qd = torch.from_numpy(q).cuda()
    any_of = torch.from_numpy(z["any"].view(np.int64).copy()).cuda()
    none_of = torch.from_numpy(z["none"].view(np.int64).copy()).cuda()
    w = torch.from_numpy(z["w"]).cuda()
    lse, cnt, bnd = sh.score_lse(qd, float(job["scale"]), weight=w, any_of=any_of, none_of=none_of)
    res = dict(lse=lse.cpu().numpy(), count=cnt.cpu().numpy(), bound=bnd.cpu().numpy())
    plain = sh.score_lse(qd, float(job["scale"]))                  # no weight, no masks
    res.update(plain_lse=plain[0].cpu().numpy(), plain_count=plain[1].cpu().numpy(), plain_bound=plain[2].cpu().numpy())
    try:
        sh.score_lse(qd, float(job["scale"]), weight=w[:-1])
        res["bad_len"] = np.array("no error")
    except ValueError as e:
        res["bad_len"] = np.array("ValueError: %s" % e)
    res["id_base_local_calls"] = np.array(h.get_counter("score_lse_calls"))
    torch.cuda.synchronize()
    h.close()
    np.savez(os.path.join(job["out_dir"], "rank%d.npz" % rank), **res)
    print("rank %d done" % rank, flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
