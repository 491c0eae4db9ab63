#!/usr/bin/env python
"""Timing of the in-batch softmax loss (csrc/inbatch_loss.hip): the head alone (sse_inbatch_loss_dev) and the full fused train
step with option train_loss 0 (pair loss) and 1 (in-batch softmax).  Writes profiles/inbatch_loss.txt (or --out).

Head: B in {128, 1024, 8192} pair rows x the encoding sizes of BASELINE.json's configs (64: the reference default, 256: the
dual-encoder configs, 512: the CNN config), random encodings, every row distinct, half the labels 1.  Each figure is the median
of REPS timed batches of CALLS back-to-back calls between two HIP events (after WARM untimed calls), with the smallest and
largest batch beside it.  Arithmetic counted: 2 B^2 S flop per logit pass and per gradient GEMM -- 3 logit passes + 2 gradient
GEMMs = 10 B^2 S useful flop per call (forward only: 2 B^2 S); the share of the 157 TFLOP/s fp32 matrix peak is of that useful
count.  The gradient passes recompute their logit tile once per 128 columns of S, which the useful count leaves out.

Step: sse_train_step of the flagship shape of bench.py (V 32000, E 50, H 256, S 256, T 32) at 8192 pair rows and of the
reference's default shape (E 50, H 96, S 64, T 80, 128 pair rows), paired batches, wall time of the synchronous call."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sse_amd  # noqa: E402

PEAK_TFLOPS = 157.3
WARM, REPS = 3, 7


def spread(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def head_times(h, B, S, grads):
    import torch
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(B * 1000 + S)
    s = torch.randn(B, S, device=dev, generator=g)
    t = 0.3 * s + torch.randn(B, S, device=dev, generator=g)
    z = (torch.arange(B, device=dev) % 2 == 0).float()
    ds, dt = (torch.empty(B, S, device=dev), torch.empty(B, S, device=dev)) if grads else (None, None)
    rl, ra = torch.empty(B, device=dev), torch.empty(B, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    calls = 20 if B <= 1024 else 3

    def call():
        h.inbatch_loss_dev(s, t, z, None, None, B, S, 64.0, 1.0 / B, ds, dt, rl, ra, st)
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


def step_times(V, E, H, S, T, B, loss, steps):
    params = dict(forward_only=False, network_mode="dual-encoder", predict_nbest=10, max_seq_length=T, vocab_size=V,
                  embedding_size=E, encoding_size=S, src_cell_size=H, tgt_cell_size=H, learning_rate=0.9,
                  learning_rate_decay_factor=0.99, targetSpaceSize=571)
    m = sse_amd.SSEModel(params)
    m.init_variables(seed=0)
    m.handle.set_option("train_loss", loss)
    rng = np.random.RandomState(0)
    src = np.repeat(rng.randint(2, V, size=(B // 2, T)).astype(np.int32), 2, axis=0)
    tgt = rng.randint(2, V, size=(B, T)).astype(np.int32)
    z = np.tile(np.array([1.0, 0.0], np.float32), B // 2)
    for _ in range(WARM):
        m.train_step(src, tgt, z)
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        m.train_step(src, tgt, z)
        out.append((time.perf_counter() - t0) * 1e3)
    assert m.handle.get_counter("train_inbatch_steps") == (WARM + steps if loss else 0)
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbatch_loss.txt"))
    ap.add_argument("--rows", default="128,1024,8192")
    ap.add_argument("--sizes", default="64,256,512")
    a = ap.parse_args()
    lines = ["in-batch softmax loss: tools/bench_inbatch_loss.py (median [min .. max] of %d timed batches, %d warm-up calls)" % (REPS, WARM), ""]
    m = sse_amd.SSEModel(dict(forward_only=False, network_mode="dual-encoder", predict_nbest=10, max_seq_length=4, vocab_size=20,
                              embedding_size=8, encoding_size=8, src_cell_size=16, tgt_cell_size=16, learning_rate=0.9,
                              learning_rate_decay_factor=0.99, targetSpaceSize=5))
    lines.append("head alone (sse_inbatch_loss_dev), ms per call; useful flop = 10 B^2 S (forward only: 2 B^2 S); peak %.1f TFLOP/s fp32 matrix" % PEAK_TFLOPS)
    lines.append("%6s %5s | %-32s %8s %6s | %-32s %8s %6s" % ("B", "S", "loss + gradients", "TFLOP/s", "peak", "forward only", "TFLOP/s", "peak"))
    for B in (int(x) for x in a.rows.split(",")):
        for S in (int(x) for x in a.sizes.split(",")):
            row = "%6d %5d |" % (B, S)
            for grads, flop in ((True, 10.0 * B * B * S), (False, 2.0 * B * B * S)):
                med, lo, hi = head_times(m.handle, B, S, grads)
                tf = flop / (med * 1e-3) / 1e12
                row += " %-32s %8.2f %5.1f%% |" % ("%.4f [%.4f .. %.4f]" % (med, lo, hi), tf, 100 * tf / PEAK_TFLOPS)
            lines.append(row.rstrip(" |"))
            print(lines[-1], flush=True)
    lines += ["", "full fused train step (sse_train_step, paired batch), ms per step, train_loss 0 = pair loss, 1 = in-batch softmax"]
    for name, shape, steps in (("flagship V 32000 E 50 H 256 S 256 T 32, 8192 pair rows", (32000, 50, 256, 256, 32, 8192), 11),
                               ("reference default E 50 H 96 S 64 T 80, 128 pair rows", (32000, 50, 96, 64, 80, 128), 31)):
        for loss in (0, 1, 0, 1):                  # each twice: the spread between two runs of the same configuration
            med, lo, hi = step_times(*shape, loss=loss, steps=steps)
            lines.append("%-58s train_loss %d: %.3f [%.3f .. %.3f]" % (name, loss, med, lo, hi))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
