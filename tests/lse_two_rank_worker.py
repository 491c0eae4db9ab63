"""One rank of tests/test_gpu_lse_two_ranks.py: `python lse_two_rank_worker.py JOB.json RANK`.

A fresh process that joins a `gloo` group on 127.0.0.1 with its peer, both on device 0 (the collectives are staged through the
host, sse_amd/collectives.py), holds ITS rows, tag words and bias values of the index only, runs ShardedIndex.score_lse and
writes rank<RANK>.npz.  It asserts nothing about numbers: the parent does."""
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
    sh.set_local_bias(torch.from_numpy(z["bias"][sh.start:sh.end].copy()).cuda())
    qd = torch.from_numpy(q).cuda()
    any_of = torch.from_numpy(z["any"].view(np.int64).copy()).cuda()
    none_of = torch.from_numpy(z["none"].view(np.int64).copy()).cuda()
    w = torch.from_numpy(z["w"]).cuda()
    lse, cnt, bnd = sh.score_lse(qd, float(job["scale"]), weight=w, any_of=any_of, none_of=none_of)
    res = dict(lse=lse.cpu().numpy(), count=cnt.cpu().numpy(), bound=bnd.cpu().numpy())
    plain = sh.score_lse(qd, float(job["scale"]))                  # no weight, no masks
    res.update(plain_lse=plain[0].cpu().numpy(), plain_count=plain[1].cpu().numpy(), plain_bound=plain[2].cpu().numpy())
    res["bad_len"] = RW.error_text(lambda: sh.score_lse(qd, float(job["scale"]), weight=w[:-1]))
    res["id_base_local_calls"] = np.array(h.get_counter("score_lse_calls"))
    RW.finish(job, rank, res, h)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
