"""One rank of tests/test_gpu_two_ranks.py: `python two_rank_worker.py JOB.json RANK`.

A fresh process (the pytest process has initialised the GPU already) that joins a `gloo` group on 127.0.0.1 with its
peers, all on device 0, builds its model with tests.util.make_pair (the same seed on every rank), runs every case of the
job in order through the product's ShardedIndex / DataParallelTrainer and writes <case>_rank<RANK>.npz.  It asserts
nothing about numbers: the parent does."""
import contextlib
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _side_stream(torch, wanted):
    """A fresh side stream when the case asks for one (its calls then run inside `with torch.cuda.stream(side)`)."""
    if not wanted:
        return None
    torch.cuda.synchronize()                                # inputs were uploaded on the default stream
    return torch.cuda.Stream()


def _on(torch, side):
    return torch.cuda.stream(side) if side is not None else contextlib.nullcontext()


def run_sharded(c, z, rank, world):
    import torch
    import sse_amd
    from tests.util import make_pair, model_params
    cid, k, N = c["id"], c["k"], c["N"]
    t, q = z[cid + "/t"], z[cid + "/q"]
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, c["S"], 4))
    h = m.handle
    sh = sse_amd.ShardedIndex(h, rank, world, N)
    assert (sh.start, sh.end) == tuple(c["bounds"][rank])
    rows = torch.from_numpy(t[sh.start:sh.end].copy()).cuda()       # this rank's rows only
    qd = torch.from_numpy(q).cuda()
    res = {}
    side = _side_stream(torch, c.get("side_stream"))
    with _on(torch, side):
        sh.set_local_rows(rows)
        for bf in c["score_bf16"]:
            h.set_option("score_bf16", bf)
            s, i = sh.score_topk(qd, k, block=c["block"])
            res["s%d" % bf], res["i%d" % bf] = s.cpu().numpy(), i.cpu().numpy()
        h.set_option("score_bf16", 0)
        try:
            sh.score_topk(qd, N + 1, block=c["block"])
            res["k_too_large"] = np.array("no error")
        except ValueError as e:
            res["k_too_large"] = np.array("ValueError: %s" % e)
        if c.get("gather_lists"):                                       # all_gather_topk on this shard's own device lists
            Q = q.shape[0]
            ls = torch.empty((Q, k), dtype=torch.float64, device="cuda")
            li = torch.empty((Q, k), dtype=torch.int64, device="cuda")
            h.score_topk_dev(qd.data_ptr(), Q, k, ls.data_ptr(), li.data_ptr(), torch.cuda.current_stream().cuda_stream)
            gs, gi = sse_amd.all_gather_topk(ls, li)
            res["gs"], res["gi"] = gs.cpu().numpy(), gi.cpu().numpy()
    torch.cuda.synchronize()
    h.close()
    return res


class ArenaTap(object):
    """The HIP handle as the trainer's engine, with the arena copied to the host just before train_apply: what the
    exchange left there, on this rank."""

    def __init__(self, handle):
        self._handle, self.trainer, self.arenas = handle, None, []

    def __getattr__(self, name):
        return getattr(self._handle, name)

    def train_apply(self):
        self.arenas.append(self.trainer.arena.cpu().numpy().copy())
        return self._handle.train_apply()


def run_dp(c, z, rank, world):
    import torch
    import sse_amd
    from tests.util import make_pair, model_params, split_arena
    cid = c["id"]
    params = model_params(c["mode"], c["V"], c["E"], c["Hs"], c["Ht"], c["S"], c["T"], N=c["N"], lr=0.9)
    m, _ = make_pair(params, seed=c["seed"])
    tap = ArenaTap(m.handle)
    tr = sse_amd.DataParallelTrainer(tap, device="cuda:0", sparse_embedding=c["sparse"])
    tap.trainer = tr
    if c["by_rows"]:
        m.handle.corpus_upload(0, z[cid + "/corpus_src"])
        m.handle.corpus_upload(1, z[cid + "/corpus_tgt"])
    res = {}
    for n, v in m.get_variables(with_slots=True).items():
        res["v0/" + n] = v
    hist, kinds = [], []
    side = _side_stream(torch, c.get("side_stream"))
    for step in range(c["steps"]):
        key = "%s/step%d/rank%d/" % (cid, step, rank)
        with _on(torch, side):
            hist.append(tr.train_step(z[key + "src"], z[key + "tgt"], z[key + "z"], rows_global=c["rows_global"][step],
                                      by_rows=c["by_rows"]))
        kinds.append(tr.last_exchange)
        torch.cuda.synchronize()
        if step in (0, c["steps"] - 1):
            for n, v in m.get_variables(with_slots=True).items():
                res["v%d/%s" % (step + 1, n)] = v
    grads, tail = split_arena(m, tap.arenas[0])
    for n, g in grads.items():
        res["g/" + n] = g
    res["tail"] = tail
    res["hist"] = np.array(hist, np.float64)
    res["kinds"] = np.array(kinds)
    res["global_step"] = np.array(m.handle.global_step)
    if side is not None:
        m.handle.set_stream(0)
    m.handle.close()
    return res


def main(job_path, rank):
    with open(job_path) as f:
        job = json.load(f)
    z = np.load(job["inputs"])
    import torch
    import torch.distributed as dist
    world = job["world"]
    torch.cuda.set_device(0)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(job["port"]))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    run = {"sharded": run_sharded, "dp": run_dp}[job["kind"]]
    for c in job["cases"]:
        res = run(c, z, rank, world)
        np.savez(os.path.join(job["out_dir"], "%s_rank%d.npz" % (c["id"], rank)), **res)
        print("case %s rank %d done" % (c["id"], rank), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
