#!/usr/bin/env python
"""sse_score_topk_after_dev at 4096 queries x 262,144 rows x 256 (synthetic unit vectors), k = 10, no tags, with the cursor of
every query at
  (a) +inf (the first page);
  (b) its row of rank 10;
  (c) its row of rank 1000;
  (d) its median score (fp32 scores of the whole index, id 0: a cursor need not be a row),
each beside sse_score_topk_filtered_dev without a filter on the same handle -- both are two sweeps plus a select -- the two
calls ALTERNATING in one session: REPS rounds (default 7; the k = 2048 comparison: 3) of one call each after one warm-up round, device time from the
library's event timers, medians and ranges.  Then 256 queries, rows 1025 .. 2048: ONE cursor call with k = 1024 (the cursor is
the 1024th row) beside sse_score_topk_dev(k = 2048), which serves k > 1024 by float64 paging.  The report is printed and
written to OUT (default profiles/score_after.txt).
usage: bench_score_after.py [REPS] [OUT] [Q,N,S] [k]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "score_after.txt")
Q, N, S = (int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (4096, 262144, 256)
K = int(sys.argv[4]) if len(sys.argv) > 4 else 10
dev = torch.device("cuda:0")
NAMES = ("score_after_collected_rows", "score_after_bruteforce_queries")
PAGING_REPS = min(REPS, 3)   # rounds of the k = 2048 comparison: the float64 paging of score_topk takes seconds per call


def alternate(h, fa, fb, reps=REPS):
    """device times of fa and fb, one call each per round"""
    fa()
    fb()
    torch.cuda.synchronize()
    print("warm-up round done", flush=True)
    ma, mb = [], []
    for _ in range(reps):
        for fn, ms in ((fa, ma), (fb, mb)):
            h.timer_record(0)
            fn()
            h.timer_record(1)
            ms.append(h.timer_elapsed_ms(0, 1))
    torch.cuda.synchronize()
    return np.array(ma), np.array(mb)


def line(name, ms, extra=""):
    med = float(np.median(ms))
    return "%-46s median %9.3f ms  min %9.3f  max %9.3f  spread %.1f %%  (n=%d)%s" % (
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
flt_s, flt_i, flt_c = torch.empty_like(out_s), torch.empty_like(out_i), torch.empty_like(out_c)

# the cursors: ranks 10 and 1000 from one k = 1024 call, the medians from fp32 scores in query chunks
deep = min(1024, N)
top_s = torch.empty((Q, deep), dtype=torch.float64, device=dev)
top_i = torch.empty((Q, deep), dtype=torch.int64, device=dev)
h.score_topk_dev(q.data_ptr(), Q, deep, top_s.data_ptr(), top_i.data_ptr())
h.synchronize()
med = torch.cat([torch.median(q[a:a + 256] @ t.T, dim=1).values for a in range(0, Q, 256)]).to(torch.float64)
positions = [("(a) cursor +inf (first page)", torch.full((Q,), float("inf"), dtype=torch.float64, device=dev), torch.zeros(Q, dtype=torch.int64, device=dev))]
for label, rank in (("(b) cursor = row of rank 10", 10), ("(c) cursor = row of rank 1000", 1000)):
    if rank <= deep:
        positions.append((label, top_s[:, rank - 1].contiguous(), top_i[:, rank - 1].contiguous()))
positions.append(("(d) cursor = median score of the query", med.contiguous(), torch.zeros(Q, dtype=torch.int64, device=dev)))


def filtered():
    h.score_topk_filtered_dev(q.data_ptr(), Q, K, None, None, None, 0, flt_s.data_ptr(), flt_i.data_ptr(), flt_c.data_ptr())


text = ["sse_score_topk_after_dev beside sse_score_topk_filtered_dev (no filter), Q=%d N=%d S=%d k=%d, no tags," % (Q, N, S, K),
        "%d alternating rounds after one warm-up round (device time)" % REPS]
for label, cs, ci in positions:
    def after(cs=cs, ci=ci):
        h.score_topk_after_dev(q.data_ptr(), Q, K, cs.data_ptr(), ci.data_ptr(), None, None, out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr())
    c0 = [h.get_counter(n) for n in NAMES]
    ma, mf = alternate(h, after, filtered)
    c1 = [h.get_counter(n) for n in NAMES]
    per = [(b - a) / float(REPS + 1) for a, b in zip(c0, c1)]
    overlap = ma.min() <= mf.max() and mf.min() <= ma.max()
    text.append("  " + label)
    text.append("    " + line("sse_score_topk_after_dev", ma))
    text.append("    " + line("sse_score_topk_filtered_dev, no filter", mf))
    text.append("    after / filtered (medians) = %.3f; ranges overlap: %s; per after call: rows re-scored %.0f, brute-force queries %.1f; counts all k: %s"
                % (np.median(ma) / np.median(mf), overlap, per[0], per[1], bool((out_c == K).all())))
    if label.startswith("(a)"):
        text.append("    the first page equals the filtered call bit for bit: %s"
                    % (torch.equal(out_i, flt_i) and torch.equal(out_s.view(torch.int64), flt_s.view(torch.int64))))
    if label.startswith("(b)") and K <= deep - 10:
        text.append("    the page equals columns 10 .. 10 + k of sse_score_topk_dev(k = %d) bit for bit: %s"
                    % (deep, torch.equal(out_i, top_i[:, 10:10 + K]) and torch.equal(out_s.view(torch.int64), top_s[:, 10:10 + K].contiguous().view(torch.int64))))

# rows 1025 .. 2048 of 256 queries: one cursor call against the float64 paging of score_topk
Q2 = min(256, Q)
if N >= 2048:
    big_s = torch.empty((Q2, 2048), dtype=torch.float64, device=dev)
    big_i = torch.empty((Q2, 2048), dtype=torch.int64, device=dev)
    pg_s = torch.empty((Q2, 1024), dtype=torch.float64, device=dev)
    pg_i = torch.empty((Q2, 1024), dtype=torch.int64, device=dev)
    pg_c = torch.empty(Q2, dtype=torch.int32, device=dev)
    cs, ci = top_s[:Q2, 1023].contiguous(), top_i[:Q2, 1023].contiguous()
    c0 = [h.get_counter(n) for n in NAMES]
    ma, mt = alternate(h, lambda: h.score_topk_after_dev(q.data_ptr(), Q2, 1024, cs.data_ptr(), ci.data_ptr(), None, None,
                                                         pg_s.data_ptr(), pg_i.data_ptr(), pg_c.data_ptr()),
                       lambda: h.score_topk_dev(q.data_ptr(), Q2, 2048, big_s.data_ptr(), big_i.data_ptr()), reps=PAGING_REPS)
    c1 = [h.get_counter(n) for n in NAMES]
    per = [(b - a) / float(PAGING_REPS + 1) for a, b in zip(c0, c1)]
    same = torch.equal(pg_i, big_i[:, 1024:]) and torch.equal(pg_s.view(torch.int64), big_s[:, 1024:].contiguous().view(torch.int64))
    text.append("  rows 1025 .. 2048 of %d queries" % Q2)
    text.append("    " + line("sse_score_topk_after_dev, k = 1024, one call", ma))
    text.append("    " + line("sse_score_topk_dev, k = 2048", mt))
    text.append("    after / score_topk (medians) = %.4f; per after call: rows re-scored %.0f, brute-force queries %.1f; the page equals columns 1024 .. 2048 bit for bit: %s"
                % (np.median(ma) / np.median(mt), per[0], per[1], same))
text = "\n".join(text) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
h.close()
