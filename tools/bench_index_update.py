#!/usr/bin/env python
"""sse_index_update_dev / sse_index_append_dev beside what a caller had to do before them, on one handle: N x S rows
(default 1.25 M x 256, synthetic unit vectors) with tags, group keys, bias and a built bf16 image (idxp16).
  existing path: sse_index_set_dev of the final rows + the three _dev setters + the first bf16 top-k call (it rebuilds idxp16);
  new path:      one sse_index_update_dev (rows and all three columns) of M = 1, 1 000, 39 000 rows, or one
                 sse_index_append_dev of 1 000 rows, + the same top-k call (idxp16 patched, not rebuilt).  The first
                 update after an upload also builds the per-row norms from idxp (one read of the index); the same update
                 a second time and the top-k call alone are timed beside it.
Both end in the same scoring call, whose results are compared (they must be equal: the final index is the same).  Device time
between two of the library's event records on the null stream, in this process, REPS alternating rounds after a warm-up
round; median, min, max.  Condition recorded: for M <= N / 32 the update is faster than the existing path.
usage: bench_index_update.py [REPS] [OUT] [N,S]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "index_update.txt")
N, S = (int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (1250000, 256)
Q, K = 64, 10
dev = torch.device("cuda:0")

params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=4, vocab_size=50,
              embedding_size=8, encoding_size=S, src_cell_size=16, tgt_cell_size=16, learning_rate=0.9,
              learning_rate_decay_factor=0.99, targetSpaceSize=5)
h = sse_amd.SSEModel(params).handle
g = torch.Generator(device=dev).manual_seed(1)
MAXM = 39000
rows = torch.nn.functional.normalize(torch.randn((N + 1000, S), generator=g, device=dev), dim=1)
fresh = torch.nn.functional.normalize(torch.randn((MAXM, S), generator=g, device=dev), dim=1)
q = torch.nn.functional.normalize(torch.randn((Q, S), generator=g, device=dev), dim=1)
tags = torch.randint(1, 255, (N + 1000,), generator=g, device=dev, dtype=torch.int64)
groups = torch.randint(0, 1000, (N + 1000,), generator=g, device=dev, dtype=torch.int64)
bias = (torch.rand((N + 1000,), generator=g, device=dev) - 0.5).contiguous()
out = [(torch.empty((Q, K), dtype=torch.float64, device=dev), torch.empty((Q, K), dtype=torch.int64, device=dev)) for _ in range(2)]


def topk(o):
    h.score_topk_dev(q.data_ptr(), Q, K, o[0].data_ptr(), o[1].data_ptr())


def existing(n):
    h.index_set_dev(rows.data_ptr(), n, S)
    h.index_set_tags_dev(tags.data_ptr(), n)
    h.index_set_groups_dev(groups.data_ptr(), n)
    h.index_set_bias_dev(bias.data_ptr(), n)
    topk(out[0])


def timed(fn):
    h.timer_record(0)
    fn()
    h.timer_record(1)
    return h.timer_elapsed_ms(0, 1)


def line(name, ms):
    ms = np.array(ms)
    return "%-44s median %9.3f ms  min %9.3f  max %9.3f  (n=%d)" % (name, float(np.median(ms)), ms.min(), ms.max(), len(ms))


text = ["index updates beside a re-upload, N=%d S=%d, tags + keys + bias set, idxp16 built; %d alternating rounds after one "
        "warm-up round (device time between event records, null stream)" % (N, S, REPS)]
for what, M in (("update", 1), ("update", 1000), ("update", MAXM), ("append", 1000)):
    if what == "update":
        ids = torch.sort(torch.randperm(N, generator=g, device=dev)[:M])[0].contiguous()
        n_final = N
    else:
        n_final = N + M
    ms_old, ms_new, ms_again, ms_topk = [], [], [], []
    for rep in range(REPS + 1):
        # the state both paths start from: the index before the change, everything built
        existing(N)
        torch.cuda.synchronize()
        if what == "update":
            t_tags, t_groups, t_bias = tags[ids].contiguous(), groups[ids].contiguous(), bias[ids].contiguous()
            new = lambda: (h.index_update_dev(ids.data_ptr(), fresh.data_ptr(), M, t_tags.data_ptr(), t_groups.data_ptr(),
                                              t_bias.data_ptr()), topk(out[1]))
        else:
            new = lambda: (h.index_append_dev(rows[N:].data_ptr(), M, tags[N:].data_ptr(), groups[N:].data_ptr(),
                                              bias[N:].data_ptr()), topk(out[1]))
        t_new = timed(new)
        torch.cuda.synchronize()
        got = (out[1][0].clone(), out[1][1].clone())
        # steady state: the same update once more (the per-row norms exist now), and the scoring call alone
        t_again = timed(new) if what == "update" else float("nan")
        t_topk = timed(lambda: topk(out[1]))
        torch.cuda.synchronize()
        # the existing path to the same final index
        if what == "update":
            rows[ids] = fresh[:M]
        torch.cuda.synchronize()
        t_old = timed(lambda: existing(n_final))
        torch.cuda.synchronize()
        same = bool(torch.equal(got[0], out[0][0]) and torch.equal(got[1], out[0][1]))
        if rep:
            ms_old.append(t_old)
            ms_new.append(t_new)
            ms_again.append(t_again)
            ms_topk.append(t_topk)
        assert same, "the two paths answer differently"
    text.append("  %s of M = %d rows (%s N / 32)" % (what, M, "<=" if M <= N // 32 else ">"))
    text.append("    " + line("existing: set_dev + 3 setters + bf16 top-k", ms_old))
    text.append("    " + line("new: one %s_dev + the same top-k" % what, ms_new))
    if what == "update":
        text.append("    " + line("new, a second time (per-row norms built)", ms_again))
    text.append("    " + line("the top-k call alone", ms_topk))
    ratio = float(np.median(ms_old) / np.median(ms_new))
    text.append("    existing / new: %.1f x; results equal" % ratio)
    if M <= N // 32:
        assert ratio > 1.0, "an update of M <= N / 32 rows slower than the re-upload"
# the host forms (synchronous: wall time): what crosses the host link is M rows instead of N
import time  # noqa: E402
rows_h = rows[:N].cpu().numpy()
tags_h, groups_h, bias_h = tags[:N].cpu().numpy().view(np.uint64), groups[:N].cpu().numpy(), bias[:N].cpu().numpy()
q_h = q.cpu().numpy()
for M in (1, 1000, MAXM):
    ids_h = np.sort(np.random.RandomState(M).choice(N, size=M, replace=False)).astype(np.int64)
    new_h = fresh[:M].cpu().numpy()
    ms_old, ms_new = [], []
    for rep in range(3):
        h.index_upload(rows_h)
        h.index_set_tags(tags_h)
        h.index_set_groups(groups_h)
        h.index_set_bias(bias_h)
        h.score_topk(q_h, K)
        t0 = time.perf_counter()
        h.index_update(ids_h, new_h, tags_h[ids_h], groups_h[ids_h], bias_h[ids_h])
        got = h.score_topk(q_h, K)
        ms_new.append(1e3 * (time.perf_counter() - t0))
        rows_h[ids_h] = new_h
        t0 = time.perf_counter()
        h.index_upload(rows_h)
        h.index_set_tags(tags_h)
        h.index_set_groups(groups_h)
        h.index_set_bias(bias_h)
        want = h.score_topk(q_h, K)
        ms_old.append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the two host paths answer differently"
    text.append("  host forms, update of M = %d rows (wall time, 3 rounds)" % M)
    text.append("    " + line("existing: upload + 3 setters + top-k", ms_old))
    text.append("    " + line("new: one index_update + the same top-k", ms_new))
    text.append("    existing / new: %.1f x; results equal" % float(np.median(ms_old) / np.median(ms_new)))
    print("\n".join(text[-3:]), flush=True)
    assert np.median(ms_old) > np.median(ms_new), "a host update of M <= N / 32 rows slower than the re-upload"
text.append("  counters: index_update_calls %d, index_update_rows %d, index_append_rows %d, index_grow_copies %d" % tuple(
    h.get_counter(n) for n in ("index_update_calls", "index_update_rows", "index_append_rows", "index_grow_copies")))
text = "\n".join(text) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
h.close()
