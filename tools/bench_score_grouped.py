#!/usr/bin/env python
"""sse_score_topk_grouped_dev at 4096 queries x 262,144 rows x 256, k = 10, against sse_score_topk_filtered_dev with no masks on
the same handle and index, timed in the same run (the two calls alternate inside every repetition):
  (a) synthetic unit vectors, a group per row: the score and id columns must equal the baseline's bit for bit;
  (b) the same index, random groups of 8 rows;
  (c) the classification shape: GROUPS (default 150) centres, every index row a noisy copy of one centre (about N / GROUPS rows
      per group, the group key is the centre), every query a noisy copy of a random centre.  Reports the queries per call the
      float64 sweep served (more than 4096 rows at or above the threshold).
REPS timed repetitions (default 5) after one warm-up of each call, device time from the library's event timers.  The report is
printed and written to OUT (default profiles/score_grouped.txt).
usage: bench_score_grouped.py [REPS] [OUT] [Q,N,S] [k] [GROUPS] [NOISE]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "score_grouped.txt")
Q, N, S = (int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (4096, 262144, 256)
K = int(sys.argv[4]) if len(sys.argv) > 4 else 10
GROUPS = int(sys.argv[5]) if len(sys.argv) > 5 else 150
NOISE = float(sys.argv[6]) if len(sys.argv) > 6 else 0.05     # per coordinate, beside a unit centre: |noise| = NOISE sqrt(S)
dev = torch.device("cuda:0")
NAMES = ("score_grouped_collected_rows", "score_grouped_bruteforce_queries")
BASE_NAMES = ("score_filtered_collected_rows", "score_filtered_bruteforce_queries")


def line(name, ms, extra=""):
    med = float(np.median(ms))
    return "%-52s median %9.3f ms  min %9.3f  max %9.3f  spread %.1f %%  (n=%d)%s" % (
        name, med, ms.min(), ms.max(), 100.0 * (ms.max() - ms.min()) / med, len(ms), extra)


params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=4, vocab_size=50,
              embedding_size=8, encoding_size=S, src_cell_size=16, tgt_cell_size=16, learning_rate=0.9,
              learning_rate_decay_factor=0.99, targetSpaceSize=5)
h = sse_amd.SSEModel(params).handle
g = torch.Generator(device=dev).manual_seed(1)
out_s = torch.empty((Q, K), dtype=torch.float64, device=dev)
out_i = torch.empty((Q, K), dtype=torch.int64, device=dev)
out_g = torch.empty((Q, K), dtype=torch.int64, device=dev)
out_c = torch.empty(Q, dtype=torch.int32, device=dev)
base_s = torch.empty((Q, K), dtype=torch.float64, device=dev)
base_i = torch.empty((Q, K), dtype=torch.int64, device=dev)
base_c = torch.empty(Q, dtype=torch.int32, device=dev)
text = ["sse_score_topk_grouped_dev, Q=%d N=%d S=%d k=%d, %d repetitions after one warm-up (device time); baseline = "
        "sse_score_topk_filtered_dev without masks, alternating with it" % (Q, N, S, K, REPS)]


def pair(name, q):
    """the baseline and the grouped call, alternating; returns their medians"""
    def base():
        h.score_topk_filtered_dev(q.data_ptr(), Q, K, None, None, None, 0, base_s.data_ptr(), base_i.data_ptr(), base_c.data_ptr())

    def grouped():
        h.score_topk_grouped_dev(q.data_ptr(), Q, K, None, None, out_s.data_ptr(), out_i.data_ptr(), out_g.data_ptr(), out_c.data_ptr())
    base()
    grouped()
    torch.cuda.synchronize()
    c0 = [h.get_counter(n) for n in NAMES + BASE_NAMES]
    ms = {"base": [], "grouped": []}
    for _ in range(REPS):
        for key, fn in (("base", base), ("grouped", grouped)):
            h.timer_record(0)
            fn()
            h.timer_record(1)
            ms[key].append(h.timer_elapsed_ms(0, 1))
    torch.cuda.synchronize()
    per = [(b - a) / float(REPS) for a, b in zip(c0, [h.get_counter(n) for n in NAMES + BASE_NAMES])]
    b_ms, g_ms = np.array(ms["base"]), np.array(ms["grouped"])
    ratio = float(np.median(g_ms)) / float(np.median(b_ms))
    text.append("  " + line(name + ": baseline", b_ms))
    text.append("      per call: collected rows %.0f, brute-force queries %.1f" % (per[2], per[3]))
    text.append("  " + line(name + ": grouped", g_ms))
    text.append("      per call: collected rows %.0f, brute-force queries %.1f; mean groups returned %.2f; grouped / baseline = %.2f"
                % (per[0], per[1], float(out_c.double().mean()), ratio))
    return ratio


t = torch.nn.functional.normalize(torch.randn((N, S), generator=g, device=dev), dim=1)
q = torch.nn.functional.normalize(torch.randn((Q, S), generator=g, device=dev), dim=1)
h.index_set_dev(t.data_ptr(), N, S)
keys = torch.randperm(N, generator=g, device=dev) * 7 - N      # a group per row
h.index_set_groups_dev(keys.data_ptr(), N)
ra = pair("(a) a group per row", q)
same = torch.equal(out_i, base_i) and torch.equal(out_s.view(torch.int64), base_s.view(torch.int64)) and torch.equal(out_g, keys[out_i])
keys = torch.randint(0, N // 8, (N,), generator=g, device=dev)
h.index_set_groups_dev(keys.data_ptr(), N)
rb = pair("(b) random groups of 8", q)
centres = torch.nn.functional.normalize(torch.randn((GROUPS, S), generator=g, device=dev), dim=1)
keys = torch.randint(0, GROUPS, (N,), generator=g, device=dev)
t = torch.nn.functional.normalize(centres[keys] + NOISE * torch.randn((N, S), generator=g, device=dev), dim=1)
qc = torch.randint(0, GROUPS, (Q,), generator=g, device=dev)
q2 = torch.nn.functional.normalize(centres[qc] + NOISE * torch.randn((Q, S), generator=g, device=dev), dim=1)
h.index_set_dev(t.data_ptr(), N, S)
h.index_set_groups_dev(keys.data_ptr(), N)
rc = pair("(c) %d groups of ~%d rows, noise %.3g" % (GROUPS, N // GROUPS, NOISE), q2)
own = float((out_g[:, 0] == qc).double().mean())
h.synchronize()
text.append("  grouped / baseline: (a) %.2f  (b) %.2f  (c) %.2f; (a) equals the baseline bit for bit and its group column is the "
            "key of its row: %s; (c) queries whose first group is their centre's: %.3f" % (ra, rb, rc, same, own))
text = "\n".join(text) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
h.close()
