#!/usr/bin/env python
"""sse_score_confusions_dev at 4096 queries x 262,144 rows x 256 (synthetic unit vectors), k = 10, four positives per query
(its rows of rank 5, 40 and 200 and one -1 padding: the best positive is the row of rank 5), three ways on one handle:
  (a) sse_score_confusions_dev at margin +inf (no cut: the filtered call's work plus the floor kernel);
  (b) sse_score_confusions_dev at margin 0 (the floor just under the top: 4 confusions per query);
  (c) what the floor form replaces: sse_score_rank_dev for the positives' scores, sse_score_topk_filtered_dev with
      exclude = positives, both results read back, the cut at (best positive score) - 0 on the host in numpy.
The three ALTERNATE in one session: REPS rounds (default 5) of one call each after one warm-up round.  (a) and (b) are timed
by the library's event timers (device time) and, like (c), by the host clock around the call and a synchronize (wall time: (c)
ends on the host).  The counter deltas per call stand beside each.  The report is printed and written to OUT (default
profiles/score_confusions.txt).  Whether the floor saves time is what this file records; no ratio is required.
usage: bench_score_confusions.py [REPS] [OUT] [Q,N,S] [k]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "score_confusions.txt")
Q, N, S = (int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (4096, 262144, 256)
K = int(sys.argv[4]) if len(sys.argv) > 4 else 10
dev = torch.device("cuda:0")
CF = ("score_confusions_collected_rows", "score_confusions_bruteforce_queries", "score_confusions_floor_queries")
FT = ("score_filtered_collected_rows", "score_filtered_bruteforce_queries")
RK = ("score_rank_band_rows", "score_rank_bruteforce_pairs")


def line(name, ms, extra=""):
    ms = np.array(ms)
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

deep = min(256, N)
top_s = torch.empty((Q, deep), dtype=torch.float64, device=dev)
top_i = torch.empty((Q, deep), dtype=torch.int64, device=dev)
h.score_topk_dev(q.data_ptr(), Q, deep, top_s.data_ptr(), top_i.data_ptr())
h.synchronize()
ranks = [r for r in (5, 40, 200) if r <= deep]
pos = torch.full((Q, len(ranks) + 1), -1, dtype=torch.int64, device=dev)
for j, r in enumerate(ranks):
    pos[:, j] = top_i[:, r - 1]
pos = pos.contiguous()
n_pos = pos.shape[1]

out = {name: (torch.empty((Q, K), dtype=torch.float64, device=dev), torch.empty((Q, K), dtype=torch.int64, device=dev),
              torch.empty(Q, dtype=torch.int32, device=dev), torch.empty(Q, dtype=torch.float64, device=dev),
              torch.empty(Q, dtype=torch.int64, device=dev)) for name in ("inf", "zero")}
flt_s, flt_i, flt_c = torch.empty((Q, K), dtype=torch.float64, device=dev), torch.empty((Q, K), dtype=torch.int64, device=dev), torch.empty(Q, dtype=torch.int32, device=dev)
pair_q = torch.arange(Q, dtype=torch.int32, device=dev).repeat_interleave(len(ranks)).contiguous()
pair_id = pos[:, :len(ranks)].reshape(-1).contiguous()
rk_before = torch.empty(pair_q.shape[0], dtype=torch.int64, device=dev)
rk_score = torch.empty(pair_q.shape[0], dtype=torch.float64, device=dev)
host_cut = {}


def confusions(name, margin):
    o = out[name]
    h.score_confusions_dev(q.data_ptr(), Q, K, pos.data_ptr(), n_pos, margin, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                           o[3].data_ptr(), o[4].data_ptr())


def two_calls_and_host_cut():
    h.score_rank_dev(q.data_ptr(), Q, pair_q.data_ptr(), pair_id.data_ptr(), pair_q.shape[0], None, rk_before.data_ptr(), rk_score.data_ptr())
    h.score_topk_filtered_dev(q.data_ptr(), Q, K, None, None, pos.data_ptr(), n_pos, flt_s.data_ptr(), flt_i.data_ptr(), flt_c.data_ptr())
    torch.cuda.synchronize()
    m = rk_score.cpu().numpy().reshape(Q, len(ranks)).max(axis=1)
    fs, fi, fc = flt_s.cpu().numpy(), flt_i.cpu().numpy(), flt_c.cpu().numpy()
    keep = (np.arange(K)[None, :] < fc[:, None]) & (fs >= (m - 0.0)[:, None])
    host_cut.update(scores=np.where(keep, fs, -np.inf), ids=np.where(keep, fi, np.iinfo(np.int64).max), counts=keep.sum(1).astype(np.int32), m=m)


legs = (("(a) sse_score_confusions_dev, margin +inf", lambda: confusions("inf", float("inf")), True),
        ("(b) sse_score_confusions_dev, margin 0", lambda: confusions("zero", 0.0), True),
        ("(c) score_rank_dev + score_topk_filtered_dev + host cut", two_calls_and_host_cut, False))
names = CF + FT + RK
dev_ms, wall_ms, deltas = {l[0]: [] for l in legs}, {l[0]: [] for l in legs}, {}
for rnd in range(REPS + 1):
    for label, fn, timed_on_device in legs:
        c0 = [h.get_counter(n) for n in names]                  # (synchronises)
        t0 = time.perf_counter()
        if timed_on_device:
            h.timer_record(0)
        fn()
        if timed_on_device:
            h.timer_record(1)
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        deltas[label] = [b - a for a, b in zip(c0, [h.get_counter(n) for n in names])]
        if rnd:                                                 # round 0 is the warm-up
            wall_ms[label].append(wall)
            if timed_on_device:
                dev_ms[label].append(h.timer_elapsed_ms(0, 1))
    if rnd == 0:
        print("warm-up round done", flush=True)

text = ["sse_score_confusions_dev beside the two calls and the host cut it replaces, Q=%d N=%d S=%d k=%d n_pos=%d (best positive: the row of rank %d),"
        % (Q, N, S, K, n_pos, ranks[0]), "%d alternating rounds after one warm-up round" % REPS]
for label, _, timed_on_device in legs:
    text.append("  " + label)
    if timed_on_device:
        text.append("    " + line("device time", dev_ms[label]))
    text.append("    " + line("wall time (call .. synchronize%s)" % ("" if timed_on_device else ", read-back and numpy cut"), wall_ms[label]))
    text.append("    counter deltas per call: " + ", ".join("%s %d" % (n, d) for n, d in zip(names, deltas[label]) if d))
zs, zi, zc, zm, _ = (a.cpu().numpy() for a in out["zero"])
same = np.array_equal(zi, host_cut["ids"]) and np.array_equal(zs, host_cut["scores"]) and np.array_equal(zc, host_cut["counts"]) and np.array_equal(zm, host_cut["m"])
text.append("  (b) equals (c) bit for bit (lists, counts, best positive score): %s; counts of (b): min %d max %d" % (same, zc.min(), zc.max()))
text.append("  (a) equals the filtered call of (c) bit for bit: %s"
            % (torch.equal(out["inf"][1], flt_i) and torch.equal(out["inf"][0].view(torch.int64), flt_s.view(torch.int64))))
wa, wb_, wc = (float(np.median(wall_ms[l[0]])) for l in legs)
text.append("  wall medians: (b) / (c) = %.3f, (a) / (c) = %.3f -- %s" % (
    wb_ / wc, wa / wc, "the floor form is faster than the two calls and the host cut" if wb_ < wc else "the floor form is SLOWER than the two calls and the host cut"))
text = "\n".join(text) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
h.close()
