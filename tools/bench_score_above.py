#!/usr/bin/env python
"""sse_score_above_dev at 4096 queries x 262,144 rows x 256 (synthetic unit vectors), thresholds set from a score_topk pass so
that every query has 32 matches and query 0 about 100,000:
  count-only form   beside sse_score_rank_dev with the same pairs (pair_score_in = thresholds, pair_id = INT64_MAX): the same sweep;
  list form         beside the only thing the library could do before: sse_score_rank_dev for the counts, then
                    sse_score_topk_dev with ONE k = the largest count for every query.  k is far above 1024, so every query
                    is paged by the float64 sweep, 16 columns per launch and every launch a full sweep of the index: at
                    k = 100,000 that is 6250 launches and does not end in a time a benchmark can spend.  What is timed, ONCE,
                    is that call at k = BASE_K (default 1040: 65 pages) on the first BASE_Q queries (default 64, the long query
                    among them); the line says so, and the pages of the full k are printed beside it as arithmetic, not as
                    a measurement.
REPS timed repetitions (default 5) after one warm-up, device time from the library's event timers.
usage: bench_score_above.py [REPS] [BASE_Q] [BASE_K] [Q,N,S]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BASE_Q = int(sys.argv[2]) if len(sys.argv) > 2 else 64
BASE_K = int(sys.argv[3]) if len(sys.argv) > 3 else 1040
Q, N, S = (int(v) for v in sys.argv[4].split(",")) if len(sys.argv) > 4 else (4096, 262144, 256)
LONG = min(100000, N // 2)
dev = torch.device("cuda:0")


def timed(h, fn, reps=REPS, warm=True):
    if warm:
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        h.timer_record(0)
        fn()
        h.timer_record(1)
        ms.append(h.timer_elapsed_ms(0, 1))
    torch.cuda.synchronize()
    return np.array(ms)


def line(name, ms):
    med = float(np.median(ms))
    return "%-44s median %9.3f ms  min %9.3f  max %9.3f  spread %.1f %%  (n=%d)" % (
        name, med, ms.min(), ms.max(), 100.0 * (ms.max() - ms.min()) / med, len(ms))


params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=4, vocab_size=50,
              embedding_size=8, encoding_size=S, src_cell_size=16, tgt_cell_size=16, learning_rate=0.9,
              learning_rate_decay_factor=0.99, targetSpaceSize=5)
h = sse_amd.SSEModel(params).handle
g = torch.Generator(device=dev).manual_seed(1)
t = torch.nn.functional.normalize(torch.randn((N, S), generator=g, device=dev), dim=1)
q = torch.nn.functional.normalize(torch.randn((Q, S), generator=g, device=dev), dim=1)
h.index_set_dev(t.data_ptr(), N, S)
s32 = torch.empty((Q, 32), dtype=torch.float64, device=dev)
i32 = torch.empty((Q, 32), dtype=torch.int64, device=dev)
h.score_topk_dev(q.data_ptr(), Q, 32, s32.data_ptr(), i32.data_ptr())
h.synchronize()
thr = s32[:, 31].clone()                                          # the 32nd best score: 32 matches
thr[0] = torch.sort(t @ q[0], descending=True).values[LONG - 1].double()   # query 0: about LONG matches
pair_q = torch.arange(Q, dtype=torch.int32, device=dev)
pair_id = torch.full((Q,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
before = torch.empty(Q, dtype=torch.int64, device=dev)
off = torch.empty(Q + 1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()

names = ("score_above_band_rows", "score_above_bruteforce_pairs", "score_above_long_segments")
c0 = [h.get_counter(n) for n in names]
rank_ms = timed(h, lambda: h.score_rank_dev(q.data_ptr(), Q, pair_q.data_ptr(), pair_id.data_ptr(), Q, thr.data_ptr(), before.data_ptr(), None))
count_ms = timed(h, lambda: h.score_above_dev(q.data_ptr(), Q, pair_q.data_ptr(), thr.data_ptr(), Q, 0, off.data_ptr(), None, None))
h.synchronize()
counts = off[1:] - off[:-1]
assert torch.equal(counts, before), "count-only form and sse_score_rank disagree"
total, kmax = int(off[-1].item()), int(counts.max().item())
ids = torch.empty(total, dtype=torch.int64, device=dev)
sc = torch.empty(total, dtype=torch.float64, device=dev)
list_ms = timed(h, lambda: h.score_above_dev(q.data_ptr(), Q, pair_q.data_ptr(), thr.data_ptr(), Q, total, off.data_ptr(), ids.data_ptr(), sc.data_ptr()))
h.synchronize()
c1 = [h.get_counter(n) for n in names]
calls = 2 * (REPS + 1)

bq, bk = min(BASE_Q, Q), min(BASE_K, kmax)
bs = torch.empty((bq, bk), dtype=torch.float64, device=dev)
bi = torch.empty((bq, bk), dtype=torch.int64, device=dev)
base_ms = timed(h, lambda: h.score_topk_dev(q.data_ptr(), bq, bk, bs.data_ptr(), bi.data_ptr()), reps=1, warm=False)
h.synchronize()
o = off.cpu().numpy()
ok = True
for p in range(bq):                                               # a segment and score_topk's row share their first columns
    n = min(int(o[p + 1] - o[p]), bk)
    ok = ok and torch.equal(ids[o[p]:o[p] + n], bi[p, :n]) and torch.equal(sc[o[p]:o[p] + n].view(torch.int64), bs[p, :n].view(torch.int64))
pages, pages_full = (bk + 15) // 16, (kmax + 15) // 16

print("Q=%d N=%d S=%d; counts: mean %.1f, max %d (query 0), total %d" % (Q, N, S, float(counts.double().mean()), kmax, total))
print("  " + line("sse_score_rank_dev (thresholds, counts)", rank_ms))
print("  " + line("sse_score_above_dev count-only", count_ms))
print("  " + line("sse_score_above_dev lists (cap = total)", list_ms))
print("  " + line("sse_score_topk_dev k=%d, FIRST %d QUERIES" % (bk, bq), base_ms))
print("  count-only / rank = %.3f" % (float(np.median(count_ms)) / float(np.median(rank_ms))))
print("  before this call, lists for these thresholds = rank + topk(k = max count = %d): %d pages of 16 columns where the timed call ran %d"
      " (%.1f ms per page for %d queries); NOT measured at the full k.  Lists form, all %d queries, measured: %.3f ms"
      % (kmax, pages_full, pages, float(base_ms[0]) / pages, bq, Q, float(np.median(list_ms))))
print("  per call: band rows %.1f, brute-force pairs %.2f, long segments %.2f; first columns of the first %d queries' segments equal score_topk's "
      "(ids and bits): %s" % ((c1[0] - c0[0]) / float(calls), (c1[1] - c0[1]) / float(calls), (c1[2] - c0[2]) / float(REPS + 1), bq, ok))
h.close()
