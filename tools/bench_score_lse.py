#!/usr/bin/env python
"""sse_score_lse_dev beside sse_score_rank_dev (one pair per query) on the same handle, at two shapes (synthetic unit vectors,
scale 64, no tags, no bias):
  8192 x 1,250,000 x 256      the large index
  16,491 x 32,060 x 256       the configs[2] evaluation size
sse_score_rank_dev is the same fp32 sweep with a compare-and-count epilogue: the fairest cost floor the project has for a
sweep that must look at every score.  Per shape the two calls ALTERNATE: REPS rounds (default 7) after two warm-up rounds,
device time from the library's event timers; median, min, max and spread per call, the ratio of the medians and the median of
the per-round ratios.  The lse of the first queries is checked against float64 on the device before anything is timed.  Then
the registers, scratch and occupancy of the kernels as the compiler reports them (tools/kernel_resources.sh).  The report is
printed and written to OUT (default profiles/score_lse.txt).
usage: bench_score_lse.py [REPS] [OUT] [Q,N,S;Q,N,S...]"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "score_lse.txt")
SHAPES = [tuple(int(v) for v in s.split(",")) for s in sys.argv[3].split(";")] if len(sys.argv) > 3 else [(8192, 1250000, 256), (16491, 32060, 256)]
WARM = 2
SCALE = 64.0
dev = torch.device("cuda:0")


def line(name, ms, extra=""):
    med = float(np.median(ms))
    return "%-24s median %9.3f ms  min %9.3f  max %9.3f  spread %.1f %%  (n=%d)%s" % (
        name, med, ms.min(), ms.max(), 100.0 * (ms.max() - ms.min()) / med, len(ms), extra)


text = ["sse_score_lse_dev beside sse_score_rank_dev (one pair per query), scale %g, no tags, no bias: %d alternating rounds after %d "
        "warm-up rounds (device time)" % (SCALE, REPS, WARM)]
for Q, N, S in SHAPES:
    params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=4, vocab_size=50,
                  embedding_size=8, encoding_size=S, src_cell_size=16, tgt_cell_size=16, learning_rate=0.9,
                  learning_rate_decay_factor=0.99, targetSpaceSize=5)
    h = sse_amd.SSEModel(params).handle
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.nn.functional.normalize(torch.randn((N, S), generator=g, device=dev), dim=1)
    q = torch.nn.functional.normalize(torch.randn((Q, S), generator=g, device=dev), dim=1)
    h.index_set_dev(t.data_ptr(), N, S)
    pair_q = torch.arange(Q, dtype=torch.int32, device=dev)
    pair_id = torch.randint(0, N, (Q,), generator=g, device=dev)
    lse = torch.empty(Q, dtype=torch.float64, device=dev)
    cnt = torch.empty(Q, dtype=torch.int64, device=dev)
    bnd = torch.empty(Q, dtype=torch.float64, device=dev)
    before = torch.empty(Q, dtype=torch.int64, device=dev)
    score = torch.empty(Q, dtype=torch.float64, device=dev)

    def run_lse():
        h.score_lse_dev(q.data_ptr(), Q, SCALE, None, None, None, lse.data_ptr(), cnt.data_ptr(), bnd.data_ptr())

    def run_rank():
        h.score_rank_dev(q.data_ptr(), Q, pair_q.data_ptr(), pair_id.data_ptr(), Q, None, before.data_ptr(), score.data_ptr())

    for _ in range(WARM):
        run_rank()
        run_lse()
    torch.cuda.synchronize()
    # results first: the first 64 queries against float64 on the device
    nq = min(Q, 64)
    want = torch.logsumexp(SCALE * (q[:nq].double() @ t.double().T), dim=1)
    err = (lse[:nq] - want).abs()
    assert bool((err <= bnd[:nq]).all()) and bool((cnt == N).all()), (float(err.max()), float(bnd[:nq].min()))
    ms = [[], []]
    for _ in range(REPS):
        for i, fn in enumerate((run_rank, run_lse)):
            h.timer_record(0)
            fn()
            h.timer_record(1)
            ms[i].append(h.timer_elapsed_ms(0, 1))
    torch.cuda.synchronize()
    r_ms, l_ms = np.array(ms[0]), np.array(ms[1])
    flop = 2.0 * Q * N * S
    text.append("  Q=%d N=%d S=%d  (first %d queries: |lse - float64| <= %.3e, bound %.3e)" % (Q, N, S, nq, float(err.max()), float(bnd[:nq].min())))
    text.append("    " + line("sse_score_rank_dev", r_ms, "  %.1f TFLOP/s of the sweep's 2 Q N S" % (flop / np.median(r_ms) * 1e-9)))
    text.append("    " + line("sse_score_lse_dev", l_ms, "  %.1f TFLOP/s" % (flop / np.median(l_ms) * 1e-9)))
    text.append("    lse / rank: ratio of medians %.3f, median of per-round ratios %.3f (rounds %.3f .. %.3f)"
                % (np.median(l_ms) / np.median(r_ms), np.median(l_ms / r_ms), (l_ms / r_ms).min(), (l_ms / r_ms).max()))
    h.close()
    del t, q
    torch.cuda.empty_cache()
text.append("kernel resources as the gfx950 compiler reports them (tools/kernel_resources.sh):")
for src in ("score_lse.hip", "score_rank.hip"):
    try:
        res = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(ROOT, "sequence-semantic-embedding_amd", "csrc", src)],
                             capture_output=True, text=True, timeout=300, check=True).stdout
        text += ["  " + ln for ln in res.splitlines() if "kernel" in ln or "sweep" in ln or "score_rank_kernel" in ln or "merge" in ln]
    except Exception as e:  # the compiler's report is an aid: its absence does not void the timings above
        text.append("  %s: not available (%s: %s)" % (src, type(e).__name__, e))
text = "\n".join(text) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
