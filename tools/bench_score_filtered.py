#!/usr/bin/env python
"""sse_score_topk_filtered_dev at 4096 queries x 262,144 rows x 256 (synthetic unit vectors), k = 10:
  (a) no filter (no tags, no exclusion list);
  (b) one of 8 tags per row, rows shuffled; every query asks for one tag;
  (c) the same tags with the rows GROUPED by tag and the queries ordered by the tag they ask for (a query block of 128 then
      asks for one tag and needs an eighth of the index tiles), with option score_filtered_skip = 1 and = 0;
  (d) no tags, n_excl = 16: every query excludes its 16 best rows.
Beside them, on the same handle in the same session: sse_score_rank_dev with one pair per query (ONE sweep of the same family)
and sse_score_topk_dev at the same k with score_bf16 = 0 (fp32 candidates).  REPS timed repetitions (default 5) after one
warm-up, device time from the library's event timers.  The report is printed and written to OUT (default
profiles/score_filtered.txt).
usage: bench_score_filtered.py [REPS] [OUT] [Q,N,S] [k]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "score_filtered.txt")
Q, N, S = (int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (4096, 262144, 256)
K = int(sys.argv[4]) if len(sys.argv) > 4 else 10
dev = torch.device("cuda:0")
NAMES = ("score_filtered_collected_rows", "score_filtered_bruteforce_queries", "score_filtered_tiles_skipped")


def timed(h, fn, reps=REPS):
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


def line(name, ms, extra=""):
    med = float(np.median(ms))
    return "%-52s median %9.3f ms  min %9.3f  max %9.3f  spread %.1f %%  (n=%d)%s" % (
        name, med, ms.min(), ms.max(), 100.0 * (ms.max() - ms.min()) / med, len(ms), extra)


params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=4, vocab_size=50,
              embedding_size=8, encoding_size=S, src_cell_size=16, tgt_cell_size=16, learning_rate=0.9,
              learning_rate_decay_factor=0.99, targetSpaceSize=5)
h = sse_amd.SSEModel(params).handle
g = torch.Generator(device=dev).manual_seed(1)
t = torch.nn.functional.normalize(torch.randn((N, S), generator=g, device=dev), dim=1)
q = torch.nn.functional.normalize(torch.randn((Q, S), generator=g, device=dev), dim=1)
h.index_set_dev(t.data_ptr(), N, S)
out_s = torch.empty((Q, K), dtype=torch.float64, device=dev)
out_i = torch.empty((Q, K), dtype=torch.int64, device=dev)
out_c = torch.empty(Q, dtype=torch.int32, device=dev)
one = torch.ones((), dtype=torch.int64, device=dev)
tags_shuffled = one << torch.randint(0, 8, (N,), generator=g, device=dev)
tags_grouped = one << (torch.arange(N, device=dev) * 8 // N)
any_random = one << torch.randint(0, 8, (Q,), generator=g, device=dev)
any_ordered = one << (torch.arange(Q, device=dev) * 8 // Q)
rows = []


def filtered(any_of=None, excl=None, n_excl=0):
    h.score_topk_filtered_dev(q.data_ptr(), Q, K, any_of.data_ptr() if any_of is not None else None, None,
                              excl.data_ptr() if excl is not None else None, n_excl, out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr())


def run(name, **kw):
    c0 = [h.get_counter(n) for n in NAMES]
    ms = timed(h, lambda: filtered(**kw))
    c1 = [h.get_counter(n) for n in NAMES]
    per = [(b - a) / float(REPS + 1) for a, b in zip(c0, c1)]
    rows.append((name, ms, "  per call: collected rows %.0f, brute-force queries %.1f, tiles skipped %.0f" % tuple(per)))
    return float(np.median(ms))


# the two comparisons: one sweep of the same family, and the unfiltered top-k with fp32 candidates
h.set_option("score_bf16", 0)
top_s = torch.empty((Q, 16), dtype=torch.float64, device=dev)
top_i = torch.empty((Q, 16), dtype=torch.int64, device=dev)
h.score_topk_dev(q.data_ptr(), Q, 16, top_s.data_ptr(), top_i.data_ptr())
h.synchronize()
pair_q = torch.arange(Q, dtype=torch.int32, device=dev)
pair_id = top_i[:, 0].contiguous()
before = torch.empty(Q, dtype=torch.int64, device=dev)
rank_ms = timed(h, lambda: h.score_rank_dev(q.data_ptr(), Q, pair_q.data_ptr(), pair_id.data_ptr(), Q, None, before.data_ptr(), None))
ks = torch.empty((Q, K), dtype=torch.float64, device=dev)
ki = torch.empty((Q, K), dtype=torch.int64, device=dev)
topk_ms = timed(h, lambda: h.score_topk_dev(q.data_ptr(), Q, K, ks.data_ptr(), ki.data_ptr()))
h.synchronize()

a_ms = run("(a) no filter")
same = torch.equal(out_i, ki) and torch.equal(out_s.view(torch.int64), ks.view(torch.int64))
h.index_set_tags_dev(tags_shuffled.data_ptr(), N)
b_ms = run("(b) one of 8 tags, rows shuffled", any_of=any_random)
h.index_set_tags_dev(tags_grouped.data_ptr(), N)
c1_ms = run("(c) rows grouped by tag, score_filtered_skip = 1", any_of=any_ordered)
grouped = (out_s.clone(), out_i.clone())
h.set_option("score_filtered_skip", 0)
c0_ms = run("(c) rows grouped by tag, score_filtered_skip = 0", any_of=any_ordered)
same_c = torch.equal(out_i, grouped[1]) and torch.equal(out_s.view(torch.int64), grouped[0].view(torch.int64))
h.set_option("score_filtered_skip", 1)
h.index_set_tags_dev(None, 0)
excl = top_i.contiguous()
d_ms = run("(d) n_excl = 16 (each query's 16 best rows)", excl=excl, n_excl=16)
h.synchronize()

rank_med, topk_med = float(np.median(rank_ms)), float(np.median(topk_ms))
text = ["sse_score_topk_filtered_dev, Q=%d N=%d S=%d k=%d, %d repetitions after one warm-up (device time)" % (Q, N, S, K, REPS)]
text.append("  " + line("sse_score_rank_dev, one pair per query", rank_ms))
text.append("  " + line("sse_score_topk_dev k=%d, score_bf16 = 0" % K, topk_ms))
for name, ms, extra in rows:
    text.append("  " + line(name, ms))
    text.append("      " + extra.strip())
text.append("  ratios to the rank call (one sweep): (a) %.2f  (b) %.2f  (c) skip on %.2f, skip off %.2f  (d) %.2f"
            % (a_ms / rank_med, b_ms / rank_med, c1_ms / rank_med, c0_ms / rank_med, d_ms / rank_med))
text.append("  ratios to score_topk (fp32 candidates): (a) %.2f  (b) %.2f  (c) skip on %.2f, skip off %.2f  (d) %.2f"
            % (a_ms / topk_med, b_ms / topk_med, c1_ms / topk_med, c0_ms / topk_med, d_ms / topk_med))
text.append("  (c) skip on / skip off = %.3f; results equal with the option on and off: %s; (a) equals sse_score_topk_dev bit for bit: %s"
            % (c1_ms / c0_ms, same_c, same))
text = "\n".join(text) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
h.close()
