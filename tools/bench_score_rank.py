#!/usr/bin/env python
"""sse_score_rank_dev (one label per query) beside the fp32 list sweep of the same handle -- sse_score_topk_dev with
score_bf16 = 0, k = 10: the same fp32 MFMA work plus list insertion -- at the crosslingual evaluation shape
(16,491 x 32,060 x 256) and at 8192 x 1.25 M x 256, synthetic unit vectors.  REPS timed repetitions each (default 7) after one
warm-up, device time from the library's event timers; prints median, min, max and the spread (max - min) / median of both,
and the two rank counters.  usage: bench_score_rank.py [REPS] [shape ...]   shape = Q,N,S"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
SHAPES = [tuple(int(v) for v in a.split(",")) for a in sys.argv[2:]] or [(16491, 32060, 256), (8192, 1250000, 256)]
dev = torch.device("cuda:0")


def timed(h, fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        h.timer_record(0)
        fn()
        h.timer_record(1)
        ms.append(h.timer_elapsed_ms(0, 1))
    torch.cuda.synchronize()
    return np.array(ms)


def line(name, ms):
    med = float(np.median(ms))
    return "%-34s median %8.3f ms  min %8.3f  max %8.3f  spread %.1f %%" % (name, med, ms.min(), ms.max(), 100.0 * (ms.max() - ms.min()) / med)


for Q, N, S in SHAPES:
    params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=4, vocab_size=50,
                  embedding_size=8, encoding_size=S, src_cell_size=16, tgt_cell_size=16, learning_rate=0.9,
                  learning_rate_decay_factor=0.99, targetSpaceSize=5)
    h = sse_amd.SSEModel(params).handle
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.nn.functional.normalize(torch.randn((N, S), generator=g, device=dev), dim=1)
    q = torch.nn.functional.normalize(torch.randn((Q, S), generator=g, device=dev), dim=1)
    h.index_set_dev(t.data_ptr(), N, S)
    h.set_option("score_bf16", 0)
    h.set_option("score_two_pass_rows", 0)
    pair_q = torch.arange(Q, dtype=torch.int32, device=dev)
    pair_id = torch.randint(0, N, (Q,), generator=g, device=dev, dtype=torch.int64)
    before = torch.empty(Q, dtype=torch.int64, device=dev)
    score = torch.empty(Q, dtype=torch.float64, device=dev)
    s10 = torch.empty((Q, 10), dtype=torch.float64, device=dev)
    i10 = torch.empty((Q, 10), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    band0, brute0 = h.get_counter("score_rank_band_rows"), h.get_counter("score_rank_bruteforce_pairs")
    rank_ms = timed(h, lambda: h.score_rank_dev(q.data_ptr(), Q, pair_q.data_ptr(), pair_id.data_ptr(), Q, None, before.data_ptr(), score.data_ptr()))
    band, brute = h.get_counter("score_rank_band_rows") - band0, h.get_counter("score_rank_bruteforce_pairs") - brute0
    topk_ms = timed(h, lambda: h.score_topk_dev(q.data_ptr(), Q, 10, s10.data_ptr(), i10.data_ptr()))
    h.synchronize()
    # a label inside the top 10 must have its list position as rank: a cheap end-to-end check of what was timed
    hit = (i10 == pair_id[:, None])
    ok = bool(torch.equal(before[hit.any(1)], hit.float().argmax(1)[hit.any(1)]))
    print("Q=%d N=%d S=%d, %d repetitions" % (Q, N, S, REPS))
    print("  " + line("sse_score_rank_dev (1 label/query)", rank_ms))
    print("  " + line("sse_score_topk_dev fp32 lists, k=10", topk_ms))
    print("  rank / list sweep = %.3f; band rows per call %.1f (%.2f per pair), brute-force pairs %d; labels in the top 10 agree: %s; "
          "mean rank %.1f" % (float(np.median(rank_ms)) / float(np.median(topk_ms)), band / float(REPS + 1), band / float(REPS + 1) / Q, brute, ok,
                              float(before.double().mean()) + 1.0))
    h.close()
    del t, q
    torch.cuda.empty_cache()
