#!/usr/bin/env python
"""Timing of the class softmax loss (csrc/class_loss.hip): the head alone (sse_class_loss_dev) and the whole train step of a
source-encoder-only model with option train_class_loss 1 beside the pair-loss step (option off) of the same batch.  Writes
profiles/class_loss.txt (or --out).

Shapes: B = 8192 and 128 pair rows against N = 571 (the demo's class count), 32768 and 100000 classes, at S = 64 and 256.
Head: random encodings and table, every source twice (a positive and a sampled negative row, as the reference builds its
batches), random target rows.  Each figure is the median of REPS timed batches of back-to-back calls between two HIP events
(after WARM untimed calls), with the smallest and largest batch beside it.  There is no bar.  The ratio column is the head's
time over the time its three passes' logit flops (3 x 2 B N Sp, Sp = S rounded up to 32) would take at the 147 TFLOP/s the
project has measured for v_mfma_f32_32x32x2_f32; the two gradient products (2 x 2 B N Sp more) are outside that count.

Step: sse_train_step of V 32000, E 50, T 32 with H = S (256) or H 96 (S 64), one session per shape: both handles warm, then
the median wall time of the synchronous call, pair loss and class loss alternating."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

MFMA_TFLOPS = 147.0
WARM, REPS = 3, 7


def spread(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def head_times(h, B, N, S, grads):
    import torch
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(B * 1000 + S)
    s = torch.randn(B // 2, S, device=dev, generator=g).repeat_interleave(2, dim=0).contiguous()
    t = torch.randn(N, S, device=dev, generator=g)
    y = torch.randint(0, N, (B,), device=dev, generator=g, dtype=torch.int32)
    z = (torch.arange(B, device=dev) % 2 == 0).float()
    ks = (torch.arange(B, device=dev) // 2).to(torch.int64)
    ds, dt = (torch.empty(B, S, device=dev), torch.empty(N, S, device=dev)) if grads else (None, None)
    rl, ra = torch.empty(B, device=dev), torch.empty(B, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    calls = 3 if B * N >= 1 << 26 else 20

    def call():
        h.class_loss_dev(s, t, y, z, ks, B, N, S, 64.0, 1.0 / B, ds, dt, rl, ra, st)
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return spread(out)


def step_times(V, E, H, S, T, B, N, steps):
    """((median, min, max) pair loss, the same for the class loss): two handles with the same weights, warm, alternating."""
    params = dict(forward_only=False, network_mode="source-encoder-only", predict_nbest=10, max_seq_length=T, vocab_size=V,
                  embedding_size=E, encoding_size=S, src_cell_size=H, tgt_cell_size=H, learning_rate=0.9,
                  learning_rate_decay_factor=0.99, targetSpaceSize=N)
    models = []
    for class_loss in (0, 1):
        m = sse_amd.SSEModel(params)
        m.init_variables(seed=0)
        m.handle.set_option("train_class_loss", class_loss)
        models.append(m)
    rng = np.random.RandomState(0)
    src = np.repeat(rng.randint(2, V, size=(B // 2, T)).astype(np.int32), 2, axis=0)
    tgt = rng.randint(0, N, size=B).astype(np.int32)
    z = np.tile(np.array([1.0, 0.0], np.float32), B // 2)
    for _ in range(WARM):
        for m in models:
            m.train_step(src, tgt, z)
    out = ([], [])
    for _ in range(steps):
        for m, ms in zip(models, out):
            t0 = time.perf_counter()
            m.train_step(src, tgt, z)
            ms.append((time.perf_counter() - t0) * 1e3)
    assert models[0].handle.get_counter("train_class_steps") == 0 and models[1].handle.get_counter("train_class_steps") == WARM + steps
    for m in models:
        m.handle.close()
    return spread(out[0]), spread(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_loss.txt"))
    ap.add_argument("--rows", default="8192,128")
    ap.add_argument("--classes", default="571,32768,100000")
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    shapes = [(B, N, S) for B in (int(x) for x in a.rows.split(",")) for N in (int(x) for x in a.classes.split(","))
              for S in (int(x) for x in a.sizes.split(","))]
    lines = ["class softmax loss: tools/bench_class_loss.py (median [min .. max] of %d timed batches, %d warm-up calls)" % (REPS, WARM), ""]
    m = sse_amd.SSEModel(dict(forward_only=False, network_mode="dual-encoder", predict_nbest=10, max_seq_length=4, vocab_size=20,
                              embedding_size=8, encoding_size=8, src_cell_size=16, tgt_cell_size=16, learning_rate=0.9,
                              learning_rate_decay_factor=0.99, targetSpaceSize=5))
    lines.append("head alone (sse_class_loss_dev), ms per call; ratio = time / time of 3 x 2 B N Sp flop at %.0f TFLOP/s" % MFMA_TFLOPS)
    lines.append("%6s %7s %5s | %-30s %7s | %-30s" % ("B", "N", "S", "loss + gradients", "ratio", "forward only"))
    for B, N, S in shapes:
        Sp = (S + 31) // 32 * 32
        ideal_ms = 3 * 2.0 * B * N * Sp / (MFMA_TFLOPS * 1e12) * 1e3
        med, lo, hi = head_times(m.handle, B, N, S, True)
        fmed, flo, fhi = head_times(m.handle, B, N, S, False)
        lines.append("%6d %7d %5d | %-30s %7.2f | %-30s" % (B, N, S, "%.4f [%.4f .. %.4f]" % (med, lo, hi), med / ideal_ms,
                                                           "%.4f [%.4f .. %.4f]" % (fmed, flo, fhi)))
        print(lines[-1], flush=True)
    m.handle.close()
    if not a.no_step:
        lines += ["", "whole train step (sse_train_step, source-encoder-only, V 32000 E 50 T 32, paired batch), ms per step"]
        lines.append("%6s %7s %5s %4s | %-30s | %-30s" % ("B", "N", "S", "H", "pair loss (train_class_loss 0)", "class loss (train_class_loss 1)"))
        for B, N, S in shapes:
            H = 256 if S == 256 else 96
            pair, cls = step_times(32000, 50, H, S, 32, B, N, 11 if B >= 1024 else 21)
            lines.append("%6d %7d %5d %4d | %-30s | %-30s" % (B, N, S, H, "%.3f [%.3f .. %.3f]" % pair, "%.3f [%.3f .. %.3f]" % cls))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
