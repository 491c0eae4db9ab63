#!/usr/bin/env python
"""sse_score_topk_biased_dev beside sse_score_topk_filtered_dev on the same handle, 4096 queries x 262,144 rows x 256
(synthetic unit vectors), k = 10, bias uniform in [-1, 1] (bmax = 1), weight 1 (NULL):
  (a) no tags;
  (b) one of 8 tags per row, rows shuffled; every query asks for one tag;
  (c) the same tags with the rows GROUPED by tag and the queries ordered by the tag they ask for (tile skip at work).
Per leg the two calls ALTERNATE: REPS rounds (default 7) of filtered, biased after two warm-up rounds, device time from the
library's event timers; median, min, max and spread per call, the ratio of the medians and the median of the per-round ratios.
Then, in a separate pass with the profiler on (its times are not the ones above), the device time of every kernel of one call
of each: which stage carries a difference.  The report is printed and written to OUT (default profiles/score_biased_bench.txt).
usage: bench_score_biased.py [REPS] [OUT] [Q,N,S] [k]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "score_biased_bench.txt")
Q, N, S = (int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (4096, 262144, 256)
K = int(sys.argv[4]) if len(sys.argv) > 4 else 10
WARM = 2
dev = torch.device("cuda:0")
FT = ("score_filtered_collected_rows", "score_filtered_bruteforce_queries", "score_filtered_tiles_skipped")
BS = ("score_biased_collected_rows", "score_biased_bruteforce_queries")


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
bias = torch.rand((N,), generator=g, device=dev) * 2.0 - 1.0
bias = (bias / bias.abs().max()).contiguous()              # bmax = 1
h.index_set_dev(t.data_ptr(), N, S)
h.index_set_bias_dev(bias.data_ptr(), N)
out = [(torch.empty((Q, K), dtype=torch.float64, device=dev), torch.empty((Q, K), dtype=torch.int64, device=dev),
        torch.empty(Q, dtype=torch.int32, device=dev)) for _ in range(2)]
one = torch.ones((), dtype=torch.int64, device=dev)
tags_shuffled = one << torch.randint(0, 8, (N,), generator=g, device=dev)
tags_grouped = one << (torch.arange(N, device=dev) * 8 // N)
any_random = one << torch.randint(0, 8, (Q,), generator=g, device=dev)
any_ordered = one << (torch.arange(Q, device=dev) * 8 // Q)


def filtered(any_of):
    o = out[0]
    h.score_topk_filtered_dev(q.data_ptr(), Q, K, any_of.data_ptr() if any_of is not None else None, None, None, 0,
                              o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())


def biased(any_of):
    o = out[1]
    h.score_topk_biased_dev(q.data_ptr(), Q, K, None, any_of.data_ptr() if any_of is not None else None, None,
                            o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())


def counters(names):
    return [h.get_counter(n) for n in names]


def kernel_times(fn, any_of):
    """{kernel name: device microseconds} of one call, from the profiler (a pass of its own)"""
    from torch.profiler import ProfilerActivity, profile
    fn(any_of)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(any_of)
        torch.cuda.synchronize()
    res = {}
    for ev in prof.key_averages():
        us = getattr(ev, "device_time_total", None)
        if us is None:
            us = getattr(ev, "cuda_time_total", 0.0)
        if us:
            res[ev.key] = res.get(ev.key, 0.0) + float(us)
    return res


text = ["sse_score_topk_biased_dev beside sse_score_topk_filtered_dev, Q=%d N=%d S=%d k=%d, bmax = 1, weight 1 (NULL): %d alternating "
        "rounds after %d warm-up rounds (device time)" % (Q, N, S, K, REPS, WARM)]
legs = (("(a) no tags", None, None), ("(b) one of 8 tags, rows shuffled", tags_shuffled, any_random),
        ("(c) rows grouped by tag, tile skip on", tags_grouped, any_ordered))
for name, tags, any_of in legs:
    h.index_set_tags_dev(tags.data_ptr() if tags is not None else None, N if tags is not None else 0)
    for _ in range(WARM):
        filtered(any_of)
        biased(any_of)
    torch.cuda.synchronize()
    c_ft, c_bs = counters(FT), counters(BS)
    ms = [[], []]
    for _ in range(REPS):
        for i, fn in enumerate((filtered, biased)):
            h.timer_record(0)
            fn(any_of)
            h.timer_record(1)
            ms[i].append(h.timer_elapsed_ms(0, 1))
    torch.cuda.synchronize()
    d_ft = [(b - a) / float(REPS) for a, b in zip(c_ft, counters(FT))]
    d_bs = [(b - a) / float(REPS) for a, b in zip(c_bs, counters(BS))]
    f_ms, b_ms = np.array(ms[0]), np.array(ms[1])
    text.append("  " + name)
    text.append("    " + line("sse_score_topk_filtered_dev", f_ms, "  per call: collected rows %.0f, brute-force queries %.1f, tiles skipped %.0f" % tuple(d_ft)))
    text.append("    " + line("sse_score_topk_biased_dev", b_ms, "  per call: collected rows %.0f, brute-force queries %.1f" % tuple(d_bs)))
    text.append("    biased / filtered: ratio of medians %.3f, median of per-round ratios %.3f (rounds %.3f .. %.3f)"
                % (np.median(b_ms) / np.median(f_ms), np.median(b_ms / f_ms), (b_ms / f_ms).min(), (b_ms / f_ms).max()))
    try:
        kf, kb = kernel_times(filtered, any_of), kernel_times(biased, any_of)
        text.append("    kernels of one call, profiler pass (device us): filtered total %.0f, biased total %.0f" % (sum(kf.values()), sum(kb.values())))
        for label, ks in (("filtered", kf), ("biased", kb)):
            for k_name, us in sorted(ks.items(), key=lambda kv: -kv[1])[:6]:
                text.append("      %-8s %10.0f  %s" % (label, us, k_name[:110]))
    except Exception as e:  # the profiler is an aid: its absence does not void the timings above
        text.append("    kernels of one call: profiler pass not available (%s: %s)" % (type(e).__name__, e))
h.index_set_tags_dev(None, 0)
h.synchronize()
text = "\n".join(text) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
h.close()
