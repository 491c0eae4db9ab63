#!/usr/bin/env python
"""Forward-only pair loss (sse_eval_loss_rows) beside what it is made of and what it replaces, HIP-event timing, one run:
8192 pair rows at the train leg's shape (bench.py: dual-encoder, V = 32000, E = 50, H = S = 256, T = 32), a paired batch
(rows 2i, 2i + 1 share their source, data.py:95-115) and an unpaired one.  Per batch:
    eval_loss_rows        row numbers in -> three double sums out (host buffers, one synchronisation)
    two sse_encode_dev    the same handle's bare inference encodes of the same ids, already on the device, un-normalised
                          (paired: the source side once per pair, as the evaluation runs it)
    train_step_rows       the train step of the same batch (forward with tapes + loss + BPTT + clip + Adagrad)
The bar: the evaluation is faster than the train step of the same batch.  Its overhead over the two bare encodes (row-number
upload, id gather, pair kernel, reduce, read-back, the synchronisation) is written down, not fixed in advance."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sse_amd  # noqa: E402
import torch  # noqa: E402

V, E, H, S, T = 32000, 50, 256, 256, 32
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
ITERS = 15
params = dict(forward_only=False, network_mode="dual-encoder", predict_nbest=10, max_seq_length=T, vocab_size=V,
              embedding_size=E, encoding_size=S, src_cell_size=H, tgt_cell_size=H, learning_rate=0.9,
              learning_rate_decay_factor=0.99, targetSpaceSize=571)
m = sse_amd.SSEModel(params)
m.init_variables(seed=0)
h = m.handle
dev = torch.device("cuda:0")


def timed(fn, iters=ITERS, warm=3):
    """Median milliseconds between two events around fn() on the null stream (fn's work runs on / is ordered against it)."""
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(iters):
        h.timer_record(0)
        fn()
        h.timer_record(1)
        ms.append(h.timer_elapsed_ms(0, 1))
    return float(np.median(ms))


rng = np.random.RandomState(1234)
tgt = rng.randint(2, V, size=(B, T)).astype(np.int32)
tgt[:, -1] = 1
z = np.tile(np.array([1.0, 0.0], np.float32), B // 2)
tgt_rows = np.arange(B, dtype=np.int32)
out_s = torch.empty((B, S), dtype=torch.float32, device=dev)
out_t = torch.empty((B, S), dtype=torch.float32, device=dev)
tgt_dev = torch.from_numpy(tgt).to(dev)
results = {}
for kind in ("paired", "unpaired"):
    n_src = B // 2 if kind == "paired" else B
    src = rng.randint(2, V, size=(n_src, T)).astype(np.int32)
    src[:, -1] = 1
    src_rows = np.repeat(np.arange(n_src, dtype=np.int32), 2) if kind == "paired" else np.arange(B, dtype=np.int32)
    h.corpus_upload(0, src)
    h.corpus_upload(1, tgt)
    src_dev = torch.from_numpy(src).to(dev)
    torch.cuda.synchronize()
    before = h.get_counter("eval_paired_calls")
    ev = timed(lambda: h.eval_loss_rows_sums(src_rows, tgt_rows, z))
    assert (h.get_counter("eval_paired_calls") > before) == (kind == "paired")

    def encodes():
        h.encode_dev(sse_amd._lib.SIDE_SOURCE, src_dev.data_ptr(), n_src, T, False, out_s.data_ptr())
        h.encode_dev(sse_amd._lib.SIDE_TARGET, tgt_dev.data_ptr(), B, T, False, out_t.data_ptr())
    enc = timed(encodes)
    h.synchronize()
    results[kind] = [ev, enc, src_rows, src]
for kind in ("paired", "unpaired"):                               # the train steps last: they move the weights
    h.corpus_upload(0, results[kind][3])                          # the batch the evaluation was timed on
    results[kind].append(timed(lambda: h.train_step_rows(results[kind][2], tgt_rows, z), iters=7))
print("forward-only pair loss, %d pair rows, dual-encoder V=%d E=%d H=S=%d T=%d, median of %d calls (train step: 7), HIP events"
      % (B, V, E, H, T, ITERS))
print("%-9s %16s %20s %18s %22s %18s" % ("batch", "eval_loss_rows ms", "2 x sse_encode_dev ms", "overhead ms (x)", "train_step_rows ms", "train / eval"))
for kind in ("paired", "unpaired"):
    ev, enc, _, _, tr = results[kind]
    print("%-9s %16.3f %20.3f %11.3f (%.2fx) %22.3f %17.2fx" % (kind, ev, enc, ev - enc, ev / enc, tr, tr / ev))
    assert ev < tr, "%s: the forward-only evaluation (%.3f ms) is not faster than the train step (%.3f ms)" % (kind, ev, tr)
