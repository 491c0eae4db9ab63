"""Headline encode alone (configs[1]: dual-encoder H = S = 256, E = 50, T = 32, V = 32000, 16384 dense rows), for clock64
phase builds (-DSSE_FWD_CLOCK) and rocprofv3 PMC passes of the matrix kernel with and without the x-projection table.

    python tools/bench_xt_encode.py [lstm_x_table (0|1|2), default 1] [launches, default 25] [rows, default 16384]

Prints the average encode time of the launches after the first five (HIP events of the handle).  SSE_FWD_ROWS=32|64
forces the row tile."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import sse_amd
    xt = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
    V, E, H, S, T = 32000, 50, 256, 256, 32
    params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=T, vocab_size=V,
                  embedding_size=E, encoding_size=S, src_cell_size=H, tgt_cell_size=H, learning_rate=0.9,
                  learning_rate_decay_factor=0.99, targetSpaceSize=571)
    dev = torch.device("cuda", 0)
    m = sse_amd.SSEModel(params, device=0)
    m.init_variables(seed=0)
    h = m.handle
    h.set_option("lstm_x_table", xt)
    g = torch.Generator(device=dev).manual_seed(100)
    ids = torch.randint(2, V, (B, T), generator=g, device=dev, dtype=torch.int32)
    ids[:, -1] = 1
    out = torch.empty((B, S), dtype=torch.float32, device=dev)
    warm = min(5, n - 1)
    for i in range(n):
        if i >= warm:
            h.timer_record(2 * (i - warm))
        h.encode_dev(0, ids.data_ptr(), B, T, True, out.data_ptr())
        if i >= warm:
            h.timer_record(2 * (i - warm) + 1)
    h.synchronize()
    ms = [h.timer_elapsed_ms(2 * i, 2 * i + 1) for i in range(n - warm)]
    print("encode B=%d lstm_x_table=%d rows=%s: %.4f ms avg over %d launches (min %.4f)"
          % (B, xt, os.environ.get("SSE_FWD_ROWS", "auto"), sum(ms) / len(ms), len(ms), min(ms)))


if __name__ == "__main__":
    main()
