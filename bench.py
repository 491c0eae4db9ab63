#!/usr/bin/env python
"""bench.py -- throughput of the SSE hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]         (N = 1)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1], SURVEY 8d "C2"): dual-encoder LSTM,
E=50, H=S=256, T=32, V=32000; a step = one pass of the hot path over one batch
per GPU, inputs resident in HBM:
    encode 16384 synthetic source sequences (embedding gather + 32 LSTM steps +
    projection + l2-normalise)  ->  cosine-score them against the resident
    571-target classification index (rows produced by the target encoder)  ->
    top-10 per query.
`value` = sequences encoded+ranked per second over all GPUs (weak scaling: every
rank processes its own batch against a replica of the small index; no
data-path collective).  A secondary, separately timed leg measures the
ranking-scale scoring path of configs[3] in weak form: 8192 queries against a
row-sharded synthetic index (1.25 M x 256 rows per GPU), per-shard top-10,
RCCL all-gather of the per-shard lists, k-way merge (`scoring_leg`).

A plain run sets up, warms up, times the K steps and prints the headline.  --full adds everything else, as before:
the secondary legs (the scoring leg above, split-bf16 and mid-batch encode, single-query latency, train step, recipe
shapes, text-CNN, real rows, config sweep), the CPU baseline, the oracle parity spot check and the full legs file.
--dump-outputs DIR writes the last timed step's encodings and top-10 scores / ids (rank 0) as DIR/*.npy.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

V, E, H, S, T = 32000, 50, 256, 256, 32
N_TARGETS = 571                       # classification target space, reference README.md:98
FLOP_PER_SEQ = T * 8 * H * (E + H) + 2 * H * S     # SURVEY 8d algorithmic LSTM forward flops (20.18 MFLOP)
PEAK_F32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md, v_mfma_f32_32x32x2_f32
PMC = {}


def csrc_sha():
    """Hash of the kernel sources: the tracked PMC summary (profiles/pmc_summary.json) is only quoted while it describes
    THIS code (traffic was read from a static file)."""
    import hashlib
    d = os.path.join(ROOT, "sequence-semantic-embedding_amd", "csrc")
    hsh = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h", ".cpp")):
            hsh.update(name.encode())
            hsh.update(open(os.path.join(d, name), "rb").read())
    return hsh.hexdigest()[:16]


def pmc_summary():
    """{kernel key: {...}} from the tracked rocprofv3 --pmc passes of this same command, or {} when the sources changed
    since they were collected (tools/collect_profiles.sh + tools/summarize_profiles.py)."""
    path = os.path.join(ROOT, "profiles", "pmc_summary.json")
    if not os.path.exists(path):
        return {}
    d = json.load(open(path))
    return d if d.get("csrc_sha") == csrc_sha() else {"stale": "profiles/pmc_summary.json was collected for csrc %s, this is %s"
                                                      % (d.get("csrc_sha"), csrc_sha())}


def _cpu_lstm(batch, seed=0):
    """(run, n_rows): torch.nn.LSTM on the CPU with the oracle's seed-0 weights re-laid out (same arithmetic as the
    oracle's BasicLSTMCell restatement, fused kernels) + projection + l2-normalise for `batch` rows of the configs[1] shape."""
    import numpy as np
    import torch
    from oracle import sse_oracle as O
    cfg = dict(vocab_size=V, embedding_size=E, encoding_size=S, src_cell_size=H, tgt_cell_size=H,
               network_mode="dual-encoder", targetSpaceSize=N_TARGETS)
    p = O.init_params(cfg, seed=seed)
    rng = np.random.RandomState(seed)
    ids = rng.randint(2, V, size=(batch, T)).astype(np.int32)
    ids[:, -1] = 1
    K, b = p["source_encoder/rnn/basic_lstm_cell/kernel"], p["source_encoder/rnn/basic_lstm_cell/bias"]
    lstm = torch.nn.LSTM(E, H, batch_first=True)
    order = [0, 2, 1, 3]
    W = np.concatenate([K[:, g * H:(g + 1) * H] for g in order], axis=1)
    bb = [b[g * H:(g + 1) * H].copy() for g in range(4)]
    bb[2] += 1.0
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.from_numpy(W[:E].T.copy()))
        lstm.weight_hh_l0.copy_(torch.from_numpy(W[E:].T.copy()))
        lstm.bias_ih_l0.copy_(torch.from_numpy(np.concatenate([bb[g] for g in order])))
        lstm.bias_hh_l0.zero_()
    emb = torch.from_numpy(p["word_embedding"])
    M = torch.from_numpy(p["source_encoder/src_M"])
    tid = torch.from_numpy(ids.astype(np.int64))

    def run():
        with torch.no_grad():
            out, _ = lstm(emb[tid])
            return torch.nn.functional.normalize(out[:, -1] @ M, dim=1)

    return run, (p, cfg, ids)


def busy_of(*prefixes):
    """PMC MFMA-busy shares (profiles/pmc_summary.json) of the kernels whose names start with one of the prefixes."""
    b = PMC.get("mfma_busy", {})
    return {k: v for k, v in b.items() if k.startswith(tuple(prefixes))} or None


def usable_cores():
    """Hardware threads this process may actually use: os.cpu_count() capped by the scheduler affinity and by the cgroup CPU
    quota (a container on a 256-thread host is often limited to a few cores: replicas beyond the quota only thrash)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
        except (OSError, ValueError, IndexError):
            pass
    return n


def cpu_replica_worker(batch, threads, t_start, budget_s):
    """One of the R CPU replicas of cpu_baseline (python bench.py --cpu-worker ...): `threads` torch threads, `batch`
    rows per call, timed from the common wall-clock instant t_start for budget_s seconds; prints 'rows seconds'."""
    import torch
    torch.set_num_threads(threads)
    run, _ = _cpu_lstm(batch)
    run()
    while time.time() < t_start:
        time.sleep(0.005)
    n, t0 = 0, time.time()
    while time.time() - t0 < budget_s:
        run()
        n += 1
    print("%d %.6f" % (n * batch, time.time() - t0), flush=True)


def cpu_baseline(batch=1024, budget_s=12.0):
    """The oracle (a port: TF1 cannot run) timed on ALL the host cores on a bounded sample of the same workload
    (8 of 256 threads was a generous denominator for the GPU): R = host_cores / 8 independent replicas
    (processes) of torch.nn.LSTM-CPU with 8 threads each, every replica encoding 16384 / R rows per call -- the GPU step's
    batch spread over the host -- all timed over the same wall-clock window; `value` is the aggregate.  The single-process
    figures (numpy oracle, torch with the best thread count) are kept beside it."""
    import subprocess
    import numpy as np
    import torch
    from oracle import sse_oracle as O
    host_threads = os.cpu_count() or 1
    cores = usable_cores()
    torch.set_num_threads(cores)
    run, (p, cfg, ids) = _cpu_lstm(batch)
    rng = np.random.RandomState(0)
    # numpy oracle
    t0 = time.time()
    O.encode(p, cfg, "src", ids[:256])
    np_rate = 256 / (time.time() - t0)
    # one process: pick the thread count that is fastest on this host (oversubscribing a big
    # box with one thread per core is slower for this small GEMM-per-step shape)
    best_threads, th_rate = cores, 0.0
    for nthr in sorted({cores, min(cores, 64), min(cores, 32), min(cores, 16), min(cores, 8)}, reverse=True):
        torch.set_num_threads(nthr)
        run()
        t0 = time.time()
        run()
        r = batch / (time.time() - t0)
        if r > th_rate:
            best_threads, th_rate = nthr, r
    torch.set_num_threads(best_threads)
    n, t0 = 0, time.time()
    while time.time() - t0 < budget_s * 0.25:
        run()
        n += 1
    th_rate = n * batch / (time.time() - t0)
    # all cores: R replicas x 8 threads
    thr = min(8, cores)
    R = max(1, cores // thr)
    rb = max(64, 16384 // R)
    t_start = time.time() + 6.0 + 0.08 * R          # replicas import torch and build their model first
    window = budget_s * 0.6
    env = dict(os.environ, OMP_NUM_THREADS=str(thr), MKL_NUM_THREADS=str(thr), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(rb), str(thr), repr(t_start), repr(window)],
                              stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, cwd=ROOT) for _ in range(R)]
    agg_rate, late = 0.0, 0
    for pr in procs:
        try:
            out = pr.communicate(timeout=window + 120)[0].decode().split()
            agg_rate += int(out[0]) / float(out[1])    # each replica over ITS elapsed time (whole calls overshoot the window)
        except Exception:                              # noqa: BLE001  (a replica that died or hung is not counted)
            pr.kill()
            late += 1
    # reference scorer, literal code path (sse_evaluator.py:110 np.dot f32 x f64; data_utils.py:263-267 getSortedResults =
    # argsort(-d) and -sort(-d) of every row), at the classification size and at ranking scale.  /root/reference is
    # not on the GPU box, so this is the oracle's restatement of those three lines (pinned bit for bit against the
    # reference's own outputs by tests/test_golden_scoring.py).  SURVEY 8d asks for Q=600 x N=1M (a 4.8 GB float64
    # temporary and ~2 minutes of single-threaded argsort): bounded here to Q=40 x N=1M, scores/s is per-score.
    def ref_scorer_rate(Q, N, budget):
        q = rng.standard_normal((Q, S)).astype(np.float32)
        tg = rng.standard_normal((N, S))
        t0 = time.time()
        reps = 0
        while reps == 0 or time.time() - t0 < budget:
            d = np.dot(q, tg.T)
            np.argsort(-d)
            -np.sort(-d, axis=1)
            reps += 1
        return reps * Q * N / (time.time() - t0)
    torch.set_num_threads(cores)
    score_rate = ref_scorer_rate(600, N_TARGETS, budget_s * 0.1)
    score_rate_1m = ref_scorer_rate(40, 1_000_000, 0.0)
    cpu_model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    single = max(np_rate, th_rate)
    best = max(single, agg_rate)
    return {"value": round(best, 1), "unit": "seqs/s",
            "cores": (R - late) * thr if agg_rate >= single else (best_threads if th_rate >= np_rate else cores),
            "host_cores": host_threads, "usable_cores": cores,
            "kind": "port",
            "sample": "LSTM source encoder fwd (T=32,E=50,H=S=256): %d replicas (processes) x %d torch threads, %d rows per call "
                      "each (the GPU step's 16384 rows spread over the host), common %.0f s window: %.0f seq/s aggregate; one "
                      "process: torch.nn.LSTM-CPU %.0f seq/s on %d threads (batch %d), numpy oracle %.0f seq/s; TF1 itself cannot run"
                      % (R - late, thr, rb, window, agg_rate, th_rate, best_threads, batch, np_rate),
            "replicas": R - late, "threads_per_replica": thr, "aggregate_seqs_per_s": round(agg_rate, 1),
            "single_process_seqs_per_s": round(single, 1),
            "host_cpu_model": cpu_model,
            "scoring_scores_per_s": round(score_rate, 1),
            "scoring_sample": "reference scorer code (np.dot f32xf64 + argsort + sort), Q=600 x N=571",
            "scoring_ranking_scale_scores_per_s": round(score_rate_1m, 1),
            "scoring_ranking_scale_sample": "the same code at Q=40 x N=1,000,000 x S=256 (numpy: BLAS threads for the dot, "
                                            "one thread for the sorts); compare with scoring_leg"}


def _events_ms(h, fn, n, warm=3):
    """Median-free average of n launches of fn between two HIP events on the library's stream."""
    for _ in range(warm):
        fn()
    h.timer_record(0)
    for _ in range(n):
        fn()
    h.timer_record(1)
    return h.timer_elapsed_ms(0, 1) / n


def reference_shapes_leg(sse_amd, torch, dev, rows=16384):
    """The shapes the reference's own recipes train and serve (every makefile recipe keeps the default cell size 96,
    sse_train.py:66-67): exact fp32 encode at 16384 device-resident rows, roofline = SURVEY 8d's algorithmic flops
    T*8*H*(E+H) + 2*H*S over the fp32 MFMA peak."""
    shapes = [("makefile:5,17 classification / qna defaults", "dual-encoder", 50, 96, 64, 80),
              ("configs[0] shared-encoder H=128", "shared-encoder", 50, 128, 64, 80),
              ("makefile:42 crosslingual recipe", "shared-encoder", 40, 96, 50, 50),
              ("makefile:30 ranking recipe", "dual-encoder", 30, 96, 64, 60),
              ("H=64 (VERDICT r03 item 2)", "dual-encoder", 40, 64, 50, 50)]
    out = {"rows": rows, "arithmetic": "v_mfma_f32_32x32x2_f32 (exact fp32), dense ids", "shapes": []}
    for name, mode, E2, H2, S2, T2 in shapes:
        params = dict(forward_only=True, network_mode=mode, predict_nbest=10, max_seq_length=T2, vocab_size=V,
                      embedding_size=E2, encoding_size=S2, src_cell_size=H2, tgt_cell_size=H2, learning_rate=0.9,
                      learning_rate_decay_factor=0.99, targetSpaceSize=N_TARGETS)
        m2 = sse_amd.SSEModel(params, device=dev.index)
        m2.init_variables(seed=0)
        g = torch.Generator(device=dev).manual_seed(5)
        ids = torch.randint(2, V, (rows, T2), generator=g, device=dev, dtype=torch.int32)
        ids[:, -1] = 1
        enc = torch.empty((rows, S2), dtype=torch.float32, device=dev)
        ms = _events_ms(m2.handle, lambda: m2.handle.encode_dev(0, ids.data_ptr(), rows, T2, True, enc.data_ptr()), 10)
        flop = T2 * 8 * H2 * (E2 + H2) + 2 * H2 * S2
        tf = rows * flop / (ms * 1e-3) / 1e12
        out["shapes"].append({"shape": name, "mode": mode, "E": E2, "H": H2, "S": S2, "T": T2, "encode_ms": ms,
                              "seqs_per_s": rows / (ms * 1e-3), "algorithmic_mflop_per_seq": flop / 1e6,
                              "roofline": {"kernel": "lstm_fwd_gs_kernel<%d> (gate-split, H <= 128 at 64-row tiles)" % ((H2 + 31) // 32),
                                           "bound": "mfma", "unit": "TFLOP/s", "achieved": tf,
                                           "peak": PEAK_F32_MFMA_TFLOPS, "frac": tf / PEAK_F32_MFMA_TFLOPS}})
        m2.handle.close()
    return out


CNN_T, CNN_S = 64, 512
CNN_FLOP_PER_SEQ = 2 * E * sum((CNN_T - fs + 1) * fs * nf for fs, nf in zip((2, 3, 4, 5), (256, 128, 128, 64))) + 2 * 576 * CNN_S


def cnn_leg(sse_amd, torch, np, dev, rows=16384, train_iters=5):
    """BASELINE configs[4]: text-CNN encoder (source_only_cnn, sse_model.py:179-214), T=64, S=512, E=50,
    571 target rows.  Encode of 16384 device-resident rows in exact fp32 and with option cnn_bf16 (bf16 storage, fp32
    accumulate: what configs[4] names), and the (builder-defined) train step at 1024 and 8192 pair rows in both
    arithmetics.  Algorithmic work 2E*sum((T-fs+1)*fs*nf) + 2*576*S = 11.24 MFLOP per sequence."""
    params = dict(forward_only=False, network_mode="source_only_cnn", predict_nbest=10, max_seq_length=CNN_T, vocab_size=V,
                  embedding_size=E, encoding_size=CNN_S, src_cell_size=96, tgt_cell_size=96, learning_rate=0.9,
                  learning_rate_decay_factor=0.99, targetSpaceSize=N_TARGETS)
    m = sse_amd.SSEModel(params, device=dev.index)
    m.init_variables(seed=0)
    h = m.handle
    g = torch.Generator(device=dev).manual_seed(11)
    ids = torch.randint(2, V, (rows, CNN_T), generator=g, device=dev, dtype=torch.int32)
    ids[:, -1] = 1
    enc = torch.empty((rows, CNN_S), dtype=torch.float32, device=dev)
    leg = {"config": "configs[4]: source_only_cnn T=%d S=%d E=%d, %d targets" % (CNN_T, CNN_S, E, N_TARGETS),
           "algorithmic_mflop_per_seq": CNN_FLOP_PER_SEQ / 1e6, "rows": rows}
    ms32 = _events_ms(h, lambda: h.encode_dev(0, ids.data_ptr(), rows, CNN_T, True, enc.data_ptr()), 10)
    ref = enc[:2048].clone()
    h.set_option("cnn_bf16", 1)
    ms16 = _events_ms(h, lambda: h.encode_dev(0, ids.data_ptr(), rows, CNN_T, True, enc.data_ptr()), 10)
    cos = torch.sum(enc[:2048] * ref, dim=1).min().item()
    h.set_option("cnn_bf16", 0)
    tf32 = rows * CNN_FLOP_PER_SEQ / (ms32 * 1e-3) / 1e12
    tf16 = rows * CNN_FLOP_PER_SEQ / (ms16 * 1e-3) / 1e12
    leg["encode_fp32"] = {"encode_ms": ms32, "seqs_per_s": rows / (ms32 * 1e-3),
                          "roofline": {"kernel": "conv_pool_kernel + proj_norm_kernel", "bound": "mfma", "unit": "TFLOP/s",
                                       "achieved": tf32, "peak": PEAK_F32_MFMA_TFLOPS, "frac": tf32 / PEAK_F32_MFMA_TFLOPS,
                                       "mfma_busy": busy_of("conv_pool_kernel")}}
    leg["encode_bf16"] = {"encode_ms": ms16, "seqs_per_s": rows / (ms16 * 1e-3), "min_cosine_vs_fp32_encode": cos,
                          "arithmetic": "embeddings / filters rounded to bf16, v_mfma_f32_32x32x16_bf16, fp32 accumulate; bias, ReLU, "
                                        "max-pool, l2-normalise in fp32; projection on split bf16 operands (hi + lo, three MFMAs "
                                        "per product: the fp32 projection to ~4e-6)",
                          "roofline": {"kernel": "conv_pool_bf16_kernel + proj_norm_x3_kernel", "bound": "mfma", "unit": "TFLOP/s",
                                       "achieved": tf16, "peak": 2500.0, "frac": tf16 / 2500.0,
                                       "mfma_busy": busy_of("conv_pool_bf16_kernel")}}
    rng = np.random.RandomState(3)
    leg["train"] = {}
    for bf in (0, 1):
        h.set_option("cnn_bf16", bf)
        for Bt in (1024, 8192):
            src = np.repeat(rng.randint(2, V, size=(Bt // 2, CNN_T)).astype(np.int32), 2, axis=0)
            src[:, -1] = 1
            tgt_rows = rng.randint(0, N_TARGETS, size=Bt).astype(np.int32)
            z = np.tile(np.array([1.0, 0.0], np.float32), Bt // 2)
            for _ in range(2):
                m.train_step(src, tgt_rows, z)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(train_iters):
                loss, _ = m.train_step(src, tgt_rows, z)
            torch.cuda.synchronize()
            d = (time.perf_counter() - t0) / train_iters
            # ALGORITHMIC flops of the step (what the roofline fraction is over): the convolution forward + the projection
            # forward and its two backward GEMMs.  The convolution backward after max-pooling is algorithmically 576 window
            # copies per sequence (~2 % of the forward); in bf16 mode dX is EXECUTED as a masked dense contraction on the bf16
            # pipe (cnn_dx_mfma_kernel: 108 groups x 4 tiles x hi/lo = the flops of two more forward convolutions) -- reported
            # beside, not counted as useful work.
            executed = Bt * (CNN_FLOP_PER_SEQ + 2 * 2 * 576 * CNN_S)
            dx_dense = Bt * 2.0 * (2 * 2 * 32 * 32 * 16 * 108) if bf else 0.0
            peak = 2500.0 if bf else PEAK_F32_MFMA_TFLOPS
            leg["train"]["%s_rows_%d" % ("bf16" if bf else "fp32", Bt)] = {
                "ms_per_step": d * 1e3, "pair_rows_per_s": Bt / d, "loss_last": loss,
                "input": "host ids in, loss / acc out (one synchronisation per step)",
                "roofline": {"kernel": "whole step: conv forward with arg-max tape, projection fwd (split bf16 in bf16 mode) / bwd "
                                       "(fp32 MFMA), conv backward (dX: masked dense bf16 MFMA in bf16 mode, gather kernel in fp32 "
                                       "mode; dW: pipelined window gather), clip, Adagrad", "bound": "mfma", "unit": "TFLOP/s",
                             "achieved": executed / d / 1e12, "peak": peak, "frac": executed / d / 1e12 / peak,
                             "masked_dense_dx_flop_per_step": dx_dense,
                             "mfma_busy": busy_of("conv_pool", "cnn_d", "proj_norm", "proj_bwd"),
                             "note": "algorithmic GEMM-shaped flops of the step over its wall time"}}
    h.set_option("cnn_bf16", 0)
    leg["hbm_bytes_per_launch_from_profiles"] = PMC.get("cnn_hbm_bytes_per_launch")
    h.close()
    return leg



def _oracle_encode_chunk(job):
    """Worker of oracle_encode_parallel (spawned process: numpy only, no HIP)."""
    p, cfg, side, ids = job
    from oracle import sse_oracle as O
    return O.encode(p, cfg, side, ids)


def oracle_encode_parallel(p, cfg, side, ids, procs):
    """The CPU oracle's encode over row chunks in `procs` spawned processes (rows are independent; the checker of
    realdata_leg would otherwise spend ~20 s single-threaded in numpy's elementwise gate arithmetic for 32,060 rows)."""
    import multiprocessing as mp
    import numpy as np
    procs = max(1, min(procs, 16, (len(ids) + 511) // 512))
    if any(k in ("LD_PRELOAD", "HSA_TOOLS_LIB") or k.startswith(("ROCP", "ROCPROF")) for k in os.environ):
        procs = 1        # under rocprofv3: no child processes at all (a profile run of this command hung in the worker pool)
    if procs == 1:
        return _oracle_encode_chunk((p, cfg, side, ids))
    chunks = np.array_split(ids, procs)
    # spawned workers inherit os.environ: one BLAS thread each (the workers are the parallelism), no GPU, and -- when this
    # process runs under rocprofv3 -- no profiler preload (16 children attaching the tool to the device hung a profile run)
    tool_vars = [k for k in os.environ if k in ("LD_PRELOAD", "HSA_TOOLS_LIB", "HSA_TOOLS_REPORT_LOAD_FAILURE") or k.startswith(("ROCP", "ROCPROF"))]
    env_keep = {k: os.environ.get(k) for k in ["OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "HIP_VISIBLE_DEVICES",
                                               "ROCR_VISIBLE_DEVICES"] + tool_vars}
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[k] = "1"
    os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = ""
    for k in tool_vars:
        os.environ.pop(k, None)
    try:
        with mp.get_context("spawn").Pool(procs) as pool:
            outs = pool.map(_oracle_encode_chunk, [(p, cfg, side, c) for c in chunks])
    finally:
        for k, v in env_keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return np.concatenate(outs, axis=0)


def realdata_leg(sse_amd, torch, np, dev, check_queries=2048):
    """BASELINE configs[2] on the REAL rawdata-crosslingual token rows the reference's own prepare_raw_data
    produced (tests/golden/crosslingual_full_ids.npz; makefile:42 T = 50; BASELINE: dual-encoder H = S = 256, E = 50):
    index build = encode ALL 32,060 targets (sse_index.py:66-92), evaluation = encode ALL 16,491 queries and rank each
    against the whole index, top-10 (sse_evaluator.py:103-113).  Rows are left-padded (mean 8.5 / 3.0 real tokens of 50):
    timed with the exact left-PAD prefix skip (library default) and without it; roofline fractions over the DENSE
    algorithmic flops (all T steps, what the reference executes) and over the NON-PAD steps only.  Parity inside the leg:
    top-1 ids of `check_queries` queries against the CPU oracle run on the same weights (oracle encodings of all targets
    and of the sampled queries, float64 scores), and the opt-in lstm_x3 path's top-1 against the exact fp32 path on ALL
    queries."""
    path = os.path.join(ROOT, "tests", "golden", "crosslingual_full_ids.npz")
    if not os.path.exists(path):
        return {"skipped": "tests/golden/crosslingual_full_ids.npz not found"}
    z = np.load(path)
    src_np, tgt_np = z["src_ids"].astype(np.int32), z["tgt_ids"].astype(np.int32)
    V3, T3, E3, H3, S3 = int(z["vocab_size"]), int(src_np.shape[1]), 50, 256, 256
    params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=T3, vocab_size=V3,
                  embedding_size=E3, encoding_size=S3, src_cell_size=H3, tgt_cell_size=H3, learning_rate=0.9,
                  learning_rate_decay_factor=0.99, targetSpaceSize=len(tgt_np))
    m = sse_amd.SSEModel(params, device=dev.index)
    m.init_variables(seed=0)
    h = m.handle
    NT_, NQ_ = len(tgt_np), len(src_np)
    tgt_d, src_d = torch.from_numpy(tgt_np).to(dev), torch.from_numpy(src_np).to(dev)
    tgt_e = torch.empty((NT_, S3), dtype=torch.float32, device=dev)
    src_e = torch.empty((NQ_, S3), dtype=torch.float32, device=dev)
    top_s = torch.empty((NQ_, 10), dtype=torch.float64, device=dev)
    top_i = torch.empty((NQ_, 10), dtype=torch.int64, device=dev)
    flop_step = 8 * H3 * (E3 + H3)
    dense_flop = T3 * flop_step + 2 * H3 * S3
    nonpad_t, nonpad_q = float((tgt_np != 0).sum(1).mean()), float((src_np != 0).sum(1).mean())
    # pad_skip sorts nothing on the device entry point: a 64-row tile starts at the smallest leading-PAD count of ITS rows.
    # The host-buffer entry point (sse_encode, what sse_index / Evaluator call) counting-sorts the rows by pad count first.
    leg = {"config": "configs[2]: rawdata-crosslingual real token rows, dual-encoder H=S=%d E=%d T=%d V=%d; %d targets, %d queries"
                     % (H3, E3, T3, V3, NT_, NQ_),
           "mean_non_pad_tokens": {"targets": nonpad_t, "queries": nonpad_q},
           "weights": "random-init (reference initialisers, seed 0)", "arithmetic": "exact fp32 (v_mfma_f32_32x32x2_f32)"}

    def enc_dev(side, ids_d, n, out):
        return lambda: h.encode_dev(side, ids_d.data_ptr(), n, T3, True, out.data_ptr())

    def roof(n, ms, nonpad, skipping):
        tf = n * dense_flop / (ms * 1e-3) / 1e12
        tf_np = n * (nonpad * flop_step + 2 * H3 * S3) / (ms * 1e-3) / 1e12
        r = {"kernel": "lstm_fwd_kernel", "bound": "mfma", "unit": "TFLOP/s", "peak": PEAK_F32_MFMA_TFLOPS}
        if not skipping:
            r.update({"achieved": tf, "frac": tf / PEAK_F32_MFMA_TFLOPS,
                      "basis": "dense algorithmic flops: all T steps, as the reference executes them -- and as this launch does",
                      "achieved_non_pad_steps_only": tf_np, "frac_non_pad_steps_only": tf_np / PEAK_F32_MFMA_TFLOPS})
        else:
            # with the PAD-prefix skip the dense figure is work AVOIDED, not a hardware rate (it can exceed the peak): the fraction
            # is quoted over the non-PAD steps, a lower bound of what the launch executes (a tile starts at the smallest PAD prefix
            # of its rows)
            r.update({"achieved": tf_np, "frac": tf_np / PEAK_F32_MFMA_TFLOPS,
                      "basis": "non-PAD steps + projection only: a lower bound of the flops this launch executes",
                      "dense_equivalent_tflops": tf,
                      "dense_equivalent_note": "all T steps / time: the rate a dense execution would need for the same time -- "
                                               "not a roofline fraction"})
        return r

    for skip in (0, 1):
        h.set_option("pad_skip", skip)
        ms_t = _events_ms(h, enc_dev(1, tgt_d, NT_, tgt_e), 5, warm=2)
        ms_q = _events_ms(h, enc_dev(0, src_d, NQ_, src_e), 5, warm=2)
        # host buffers in and out (PCIe-inclusive; rows counting-sorted by pad count inside the call when pad_skip = 1)
        m.encode_target(tgt_np[:4096])
        t0 = time.perf_counter()
        m.encode_target(tgt_np)
        host_t = time.perf_counter() - t0
        t0 = time.perf_counter()
        m.encode_source(src_np)
        host_q = time.perf_counter() - t0
        leg["pad_skip_%d" % skip] = {
            "index_build": {"encode_ms": ms_t, "seqs_per_s": NT_ / (ms_t * 1e-3), "roofline": roof(NT_, ms_t, nonpad_t, skip == 1),
                            "host_buffers_ms": host_t * 1e3, "host_buffers_seqs_per_s": NT_ / host_t},
            "query_encode": {"encode_ms": ms_q, "seqs_per_s": NQ_ / (ms_q * 1e-3), "roofline": roof(NQ_, ms_q, nonpad_q, skip == 1),
                             "host_buffers_ms": host_q * 1e3, "host_buffers_seqs_per_s": NQ_ / host_q}}
    # ranking: all queries against the whole index (resident, float32 rows as the device produced them)
    h.index_set_dev(tgt_e.data_ptr(), NT_, S3)
    ms_s = _events_ms(h, lambda: h.score_topk_dev(src_e.data_ptr(), NQ_, 10, top_s.data_ptr(), top_i.data_ptr()), 5, warm=2)
    leg["score"] = {"queries": NQ_, "index_rows": NT_, "k": 10, "ms_per_pass": ms_s, "scores_per_s": NQ_ * NT_ / (ms_s * 1e-3),
                    "roofline": {"kernel": "score_topk_kernel (bf16 candidates) + float64 re-scoring", "bound": "mfma", "unit": "TFLOP/s",
                                 "achieved": 2.0 * S3 * NQ_ * NT_ / (ms_s * 1e-3) / 1e12, "peak": 2500.0,
                                 "frac": 2.0 * S3 * NQ_ * NT_ / (ms_s * 1e-3) / 1e12 / 2500.0}}
    best = leg["pad_skip_1"]
    whole = best["index_build"]["encode_ms"] + best["query_encode"]["encode_ms"] + ms_s
    leg["whole_job_ms"] = whole
    leg["whole_job"] = "index build + query encode + ranking, device-resident inputs, pad_skip = 1: %.2f ms for %d + %d sequences and %.3g scores" \
                       % (whole, NT_, NQ_, float(NQ_) * NT_)
    exact_i = top_i[:, 0].clone()
    # the opt-in split-bf16 encoder on the same data: top-1 of ALL queries against the exact fp32 path
    h.set_option("lstm_x3", 1)
    tgt_x = torch.empty_like(tgt_e)
    src_x = torch.empty_like(src_e)
    ms_tx = _events_ms(h, enc_dev(1, tgt_d, NT_, tgt_x), 3, warm=1)
    ms_qx = _events_ms(h, enc_dev(0, src_d, NQ_, src_x), 3, warm=1)
    h.index_set_dev(tgt_x.data_ptr(), NT_, S3)
    xs = torch.empty_like(top_s)
    xi = torch.empty_like(top_i)
    h.score_topk_dev(src_x.data_ptr(), NQ_, 10, xs.data_ptr(), xi.data_ptr())
    h.synchronize()
    margin = (top_s[:, 0] - top_s[:, 1])
    same = (xi[:, 0] == exact_i)
    leg["lstm_x3"] = {"index_build_ms": ms_tx, "query_encode_ms": ms_qx,
                      "top1_equal_to_exact_fp32_path": int(same.sum().item()), "queries": NQ_,
                      "max_abs_encoding_diff": float(max((tgt_x - tgt_e).abs().max().item(), (src_x - src_e).abs().max().item())),
                      "max_top2_margin_among_flips": float(margin[~same].max().item()) if int((~same).sum().item()) else 0.0,
                      "note": "opt-in (option lstm_x3): three bf16 MFMAs on hi + lo split fp32 operands per product; flips can only "
                              "happen where the exact path's own top-2 margin is below the encoding difference"}
    h.set_option("lstm_x3", 0)
    h.index_set_dev(tgt_e.data_ptr(), NT_, S3)
    # parity against the CPU oracle on the same weights: its encodings of ALL targets and of a query sample
    from oracle import sse_oracle as O
    p = {k: v for k, v in m.get_variables().items()}
    nq = min(check_queries, NQ_)
    pick = np.linspace(0, NQ_ - 1, nq).astype(np.int64)
    t0 = time.perf_counter()
    procs = usable_cores()
    want_t = oracle_encode_parallel(p, params, "tgt", tgt_np, procs)
    want_q = oracle_encode_parallel(p, params, "src", src_np[pick], procs)
    wsc, wids = O.topk_fast(O.scores_f64(want_q, want_t.astype(np.float64)), 2)
    pick_d = torch.from_numpy(pick).to(dev)
    got_i = exact_i[pick_d].cpu().numpy()
    clear = (wsc[:, 0] - wsc[:, 1]) > 2e-6
    leg["parity_vs_oracle"] = {"queries_checked": int(nq), "index_rows": NT_,
                               "top1_equal": int(np.sum(got_i == wids[:, 0])),
                               "top1_equal_where_oracle_margin_gt_2e-6": "%d of %d" % (int(np.sum(got_i[clear] == wids[clear, 0])), int(clear.sum())),
                               "max_abs_encoding_err_targets": float(np.abs(tgt_e.cpu().numpy() - want_t).max()),
                               "max_abs_encoding_err_queries": float(np.abs(src_e[pick_d].cpu().numpy() - want_q).max()),
                               "oracle_seconds": time.perf_counter() - t0, "oracle_processes": procs}
    h.close()
    return leg


def config_sweep_leg(sse_amd, torch, dev, h_main, full_c4=True):
    """SURVEY 8d C2 batch sweep (both encoders of the configs[1] model, B in {1, 64, 1024, 16384, 131072}, device-resident
    dense ids) and configs[3] in full: 100,000 queries x 10,000,000 targets, k = 10, as 8 LOGICAL shards of 1.25 M rows
    scored one after the other on this GPU (id_base = shard offset) + the k-way merge the RCCL all-gather feeds; top-1
    checked against planted targets (normalize(q + 0.1 noise) at row j of shard j % 8)."""
    h = h_main
    out = {"c2_batch_sweep": [], "timing": "HIP events on the library's stream around n back-to-back calls"}
    for B in (1, 64, 1024, 16384, 131072):
        g = torch.Generator(device=dev).manual_seed(31 + B)
        ids = torch.randint(2, V, (B, T), generator=g, device=dev, dtype=torch.int32)
        ids[:, -1] = 1
        enc = torch.empty((B, S), dtype=torch.float32, device=dev)
        row = {"B": B}
        for side, name in ((0, "src"), (1, "tgt")):
            n = 100 if B <= 1024 else 10 if B <= 16384 else 3
            ms = _events_ms(h, lambda: h.encode_dev(side, ids.data_ptr(), B, T, True, enc.data_ptr()), n, warm=2)
            tf = B * FLOP_PER_SEQ / (ms * 1e-3) / 1e12
            row[name] = {"ms_per_call": ms, "seqs_per_s": B / (ms * 1e-3), "tflops": tf, "frac_of_f32_mfma_peak": tf / PEAK_F32_MFMA_TFLOPS}
        out["c2_batch_sweep"].append(row)
        del ids, enc
    if full_c4:
        Q, NS, P, k = 100000, 1250000, 8, 10
        gq = torch.Generator(device=dev).manual_seed(2)
        q = torch.nn.functional.normalize(torch.randn((Q, S), generator=gq, device=dev), dim=1)
        noise = torch.randn((Q, S), generator=gq, device=dev)
        all_s = torch.empty((P, Q, k), dtype=torch.float64, device=dev)
        all_i = torch.empty((P, Q, k), dtype=torch.int64, device=dev)
        jj = torch.arange(Q, device=dev)
        t_build = t_score = 0.0
        for p in range(P):
            g = torch.Generator(device=dev).manual_seed(100 + p)
            shard = torch.nn.functional.normalize(torch.randn((NS, S), generator=g, device=dev), dim=1)
            mine = jj[jj % P == p]
            shard[mine] = torch.nn.functional.normalize(q[mine] + 0.1 * noise[mine], dim=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.index_set_dev(shard.data_ptr(), NS, S, id_base=p * NS)
            h.synchronize()
            t1 = time.perf_counter()
            h.score_topk_dev(q.data_ptr(), Q, k, all_s[p].data_ptr(), all_i[p].data_ptr())
            h.synchronize()
            t2 = time.perf_counter()
            t_build += t1 - t0
            t_score += t2 - t1
            del shard
        out_s = torch.empty((Q, k), dtype=torch.float64, device=dev)
        out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
        t0 = time.perf_counter()
        h.merge_topk_dev(all_s.data_ptr(), all_i.data_ptr(), P, Q, k, out_s.data_ptr(), out_i.data_ptr())
        h.synchronize()
        t_merge = time.perf_counter() - t0
        tot = t_score + t_merge
        out["c4_full"] = {"queries": Q, "index_rows": NS * P, "logical_shards": P, "k": k, "S": S,
                          "score_s": t_score, "merge_s": t_merge, "total_s": tot, "index_layout_build_s": t_build,
                          "scores_per_s": float(Q) * NS * P / tot,
                          "planted_top1_acc": float((out_i[:, 0] == (jj % P) * NS + jj).double().mean().item()),
                          "rows_sorted": bool((out_s[:, :-1] >= out_s[:, 1:]).all().item()),
                          "roofline": {"kernel": "score_topk_kernel<4,true,false,true> x 8 shards + merge_topk", "bound": "mfma",
                                       "unit": "TFLOP/s", "achieved": 2.0 * S * Q * NS * P / tot / 1e12, "peak": 2500.0,
                                       "frac": 2.0 * S * Q * NS * P / tot / 1e12 / 2500.0},
                          "note": "ONE GPU doing the work of the 8 of configs[3]; on 8 GPUs each rank runs one shard's pass and the "
                                  "merge consumes the all-gathered lists"}
        del q, noise, all_s, all_i
    return out


HEADLINE_MAX_BYTES = 6000      # the driver's parser lost the 23.5 KB line of round 5
LEGS_FILE = os.path.join("profiles", "bench_legs_latest.json")


def _r(x, nd=4):
    """Round floats to nd significant digits (the headline is a summary; full precision lives in the legs file)."""
    if isinstance(x, float):
        return float("%.*g" % (nd, x)) if x == x and abs(x) != float("inf") else None
    return x


def _leg(d, ms_key, roof=None, **extra):
    """One compact number set of a secondary leg: the time, the roofline fraction, and whatever else is named."""
    if not isinstance(d, dict):
        return None
    out = {"ms": _r(d.get(ms_key))}
    r = d.get("roofline") if roof is None else roof
    if isinstance(r, dict):
        out["frac"] = _r(r.get("frac"))
        if isinstance(r.get("mfma_busy"), float):
            out["mfma_busy"] = _r(r["mfma_busy"])
    for k, v in extra.items():
        out[k] = _r(v)
    return out


def compact_headline(full, with_legs=True):
    """The ONE line the driver parses: the contract keys, `roofline` and `cpu_baseline` without prose, and one compact
    number set per secondary leg.  Everything else is in LEGS_FILE (and on the BENCH_LEGS line printed before it).
    with_legs=False (a plain run, no secondary legs): the contract keys and `roofline` only."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "cosine_scores_per_s", "top1_match_vs_oracle", "encode_max_abs_err_vs_oracle",
            "speedup_vs_cpu_baseline", "rccl_ranks_seen", "shard_bounds")
    line = {k: _r(full[k], 7) for k in keep if k in full}
    rf = full["roofline"]
    line["roofline"] = {k: _r(rf.get(k), 6) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "mfma_busy",
                                                        "avg_kernel_ms", "algorithmic_flop_per_launch", "pmc_source",
                                                        "traffic_measured_in_this_run")}
    cb = full.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: _r(cb.get(k), 6) for k in ("value", "unit", "cores", "kind", "host_cores", "replicas",
                                                               "threads_per_replica", "host_cpu_model", "scoring_scores_per_s")}
        line["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:160]
    if not with_legs:
        return json.dumps(line, separators=(",", ":"))
    legs = {}
    g = full.get
    if g("scoring_leg"):
        legs["score_bf16_sweep"] = _leg(g("scoring_leg"), "ms_per_pass", planted_top1=g("scoring_leg")["top1_planted_acc"],
                                        identical_to_fp32=g("scoring_leg")["identical_to_fp32_candidates"])
        legs["score_fp32_sweep"] = _leg(g("scoring_leg_fp32_candidates"), "ms_per_pass")
    if g("encode_leg_split_bf16"):
        legs["encode_split_bf16"] = _leg(g("encode_leg_split_bf16"), "encode_kernel_ms")
    if g("encode_leg_mid_batch"):
        for rows, d in g("encode_leg_mid_batch")["rows"].items():
            legs["encode_rows_%s" % rows] = _leg(d, "encode_ms", identical=d["identical_to_matrix_kernel"])
    if g("latency_leg"):
        la = g("latency_leg")
        legs["latency_q1"] = {k2: _r(v) for k2, v in la.items() if k2.endswith("_ms") or "_ms_" in k2}
        legs["latency_q1"]["sweep_hbm_frac"] = _r(la["roofline"]["frac"])
    if g("train_leg"):
        legs["train_fp32"] = _leg(g("train_leg"), "ms_per_step", rows=g("train_leg")["pair_rows_per_gpu"],
                                  split_bf16_ms=g("train_leg")["ms_per_step_split_bf16_opt_in"])
        if "default_shape" in g("train_leg"):
            legs["train_default_shape"] = {k2: _r(v) for k2, v in g("train_leg")["default_shape"].items()
                                           if isinstance(v, (int, float))}
    if g("encode_leg_reference_shapes"):
        legs["encode_recipe_shapes"] = [{"H": sh.get("H"), "T": sh.get("T"), "ms": _r(sh.get("encode_ms")),
                                         "frac": _r((sh.get("roofline") or {}).get("frac"))}
                                        for sh in g("encode_leg_reference_shapes")["shapes"]]
    if g("cnn_leg"):
        c = g("cnn_leg")
        legs["cnn"] = {"encode_fp32": _leg(c.get("encode_fp32"), "encode_ms"), "encode_bf16": _leg(c.get("encode_bf16"), "encode_ms")}
        for name, d in (c.get("train") or {}).items():
            if isinstance(d, dict):
                legs["cnn"]["train_" + name] = _leg(d, "ms_per_step")
    if g("realdata_leg"):
        rd = g("realdata_leg")
        out = {"whole_job_ms": _r(rd.get("whole_job_ms"))}
        for ps in ("pad_skip_0", "pad_skip_1"):
            for part in ("index_build", "query_encode"):
                d = (rd.get(ps) or {}).get(part)
                if isinstance(d, dict):
                    out["%s_%s" % (part, ps)] = _leg(d, "encode_ms")
        if isinstance(rd.get("score"), dict):
            out["score"] = _leg(rd["score"], "ms_per_pass")
        pv = rd.get("parity_vs_oracle") or {}
        out["top1_equal_vs_oracle"] = "%s/%s" % (pv.get("top1_equal"), pv.get("queries_checked"))
        legs["realdata_c3"] = out
    if g("config_sweep"):
        cs = g("config_sweep")
        legs["c2_batch_sweep"] = [{"B": e["B"], "src_ms": _r(e["src"]["ms_per_call"]),
                                   "frac": _r(e["src"].get("frac_of_f32_mfma_peak"))} for e in cs.get("c2_batch_sweep", [])]
        if cs.get("c4_full"):
            legs["c4_full_1gpu"] = {"total_s": _r(cs["c4_full"]["total_s"]), "frac": _r(cs["c4_full"]["roofline"]["frac"]),
                                    "planted_top1": cs["c4_full"]["planted_top1_acc"]}
    line["legs"] = legs
    line["legs_file"] = LEGS_FILE
    text = json.dumps(line, separators=(",", ":"))
    if len(text) > HEADLINE_MAX_BYTES:            # never let a new leg push the line past the parser again: shed legs, largest first
        for name in sorted(legs, key=lambda n: -len(json.dumps(legs[n]))):
            legs.pop(name)
            line["legs_truncated"] = True
            text = json.dumps(line, separators=(",", ":"))
            if len(text) <= HEADLINE_MAX_BYTES:
                break
    return text


def emit(full, with_legs=True):
    """Full legs -> LEGS_FILE and an earlier, non-'{'-leading stdout line; the compact headline is the LAST line.
    with_legs=False (a plain run): the headline line alone."""
    if with_legs:
        try:
            os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
            with open(os.path.join(ROOT, LEGS_FILE), "w") as f:
                json.dump(full, f, indent=1)
        except OSError:
            pass
    # RCCL (NCCL_DEBUG=VERSION on the GPU boxes) prints its banner through C stdio, which would otherwise be
    # flushed at exit, AFTER this line: push it out first so that the JSON line is the last line of stdout
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    if with_legs:
        print("BENCH_LEGS " + json.dumps(full), flush=True)
    print(compact_headline(full, with_legs=with_legs), flush=True)


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, src_enc, top_s, top_i):
    """--dump-outputs: what the timed path handed back in its last step -- the l2-normalised source encodings and the
    top-10 scores and row ids per query -- as out_dir/<name>.npy (float32 / float64; ids < 2^53 are exact in float64).
    When the batch would take more than DUMP_MAX_BYTES, the same fixed, seeded sample of rows is written from every
    array, and its row numbers as sample_rows.npy."""
    import numpy as np
    arrays = {"src_enc": src_enc.cpu().numpy().astype(np.float32),
              "top_scores": top_s.cpu().numpy().astype(np.float64),
              "top_ids": top_i.cpu().numpy().astype(np.float64)}
    rows = arrays["src_enc"].shape[0]
    per_row = sum(a[0].nbytes for a in arrays.values())
    if rows * per_row > DUMP_MAX_BYTES:
        keep = np.sort(np.random.RandomState(0).choice(rows, (DUMP_MAX_BYTES - 4096) // (per_row + 8), replace=False))
        arrays = {k: a[keep] for k, a in arrays.items()}
        arrays["sample_rows"] = keep.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16384, help="source sequences per GPU per step")
    ap.add_argument("--score-rows", type=int, default=1250000, help="scoring leg: index rows per GPU")
    ap.add_argument("--score-queries", type=int, default=8192)
    ap.add_argument("--score-iters", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-scoring-leg", action="store_true")
    ap.add_argument("--train-rows", type=int, default=8192, help="train leg: pair rows per GPU per step")
    ap.add_argument("--train-iters", type=int, default=5)
    ap.add_argument("--no-train-leg", action="store_true")
    ap.add_argument("--no-x3-leg", action="store_true")
    ap.add_argument("--no-cnn-leg", action="store_true")
    ap.add_argument("--no-shapes-leg", action="store_true")
    ap.add_argument("--no-realdata-leg", action="store_true")
    ap.add_argument("--no-sweep-leg", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary legs, the CPU baseline and the oracle parity check, and write the full legs "
                         "to %s; a plain run times the headline steps only" % LEGS_FILE)
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last step computed (encodings, top-10 scores and ids) to DIR/*.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:               # a plain run: setup, warm-up, the timed steps, the outputs, the headline line
        for leg in ("cpu_baseline", "scoring_leg", "train_leg", "x3_leg", "cnn_leg", "shapes_leg", "realdata_leg", "sweep_leg"):
            setattr(args, "no_" + leg, True)

    global PMC
    PMC = pmc_summary()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d"
                         % (args.gpus, world, args.gpus))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    import numpy as np
    import torch
    import torch.distributed as dist
    import sse_amd

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # SSE_BENCH_FORCE_DIST=1: run every N>1 code path (process group, barriers, max-over-ranks, all-gather + merge,
    # gradient all-reduce) in a 1-rank RCCL group -- a single-GPU box can then check the multi-GPU branches
    force_dist = os.environ.get("SSE_BENCH_FORCE_DIST") == "1"
    use_dist = world > 1 or force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # proof that RCCL saw every rank: an all-reduce of ones over the job's process group
    rccl_ranks_seen = 1
    if use_dist and args.full:
        ones = torch.ones(1, dtype=torch.float32, device=dev)
        dist.all_reduce(ones)
        rccl_ranks_seen = int(ones.item())

    params = dict(forward_only=True, network_mode="dual-encoder", predict_nbest=10, max_seq_length=T,
                  vocab_size=V, embedding_size=E, encoding_size=S, src_cell_size=H, tgt_cell_size=H,
                  learning_rate=0.9, learning_rate_decay_factor=0.99, targetSpaceSize=N_TARGETS)
    m = sse_amd.SSEModel(params, device=local_rank)
    m.init_variables(seed=0)                     # same weights on every rank
    h = m.handle

    # ---- the resident target index: 571 synthetic target sequences through the target encoder
    g = torch.Generator(device=dev).manual_seed(1234)
    tgt_ids = torch.randint(2, V, (N_TARGETS, T), generator=g, device=dev, dtype=torch.int32)
    tgt_ids[:, -1] = 1
    tgt_enc = torch.empty((N_TARGETS, S), dtype=torch.float32, device=dev)
    h.encode_dev(1, tgt_ids.data_ptr(), N_TARGETS, T, True, tgt_enc.data_ptr())
    h.index_set_dev(tgt_enc.data_ptr(), N_TARGETS, S)

    # ---- this rank's query batch (synthetic ids, dense: no padding, EOS last)
    B = args.batch
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    src_ids = torch.randint(2, V, (B, T), generator=g, device=dev, dtype=torch.int32)
    src_ids[:, -1] = 1
    src_enc = torch.empty((B, S), dtype=torch.float32, device=dev)
    top_s = torch.empty((B, 10), dtype=torch.float64, device=dev)
    top_i = torch.empty((B, 10), dtype=torch.int64, device=dev)

    def step(record=None):
        if record is not None:
            h.timer_record(2 * record)
        h.encode_dev(0, src_ids.data_ptr(), B, T, True, src_enc.data_ptr())
        if record is not None:
            h.timer_record(2 * record + 1)
        h.score_topk_dev(src_enc.data_ptr(), B, 10, top_s.data_ptr(), top_i.data_ptr())

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    nrec = min(args.steps, 100)
    for i in range(args.steps):
        step(i if i < nrec else None)
    barrier()
    dt = time.perf_counter() - t0
    h.synchronize()
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    enc_ms = [h.timer_elapsed_ms(2 * i, 2 * i + 1) for i in range(nrec)]
    enc_ms_avg = sum(enc_ms) / len(enc_ms)

    value = world * B * args.steps / dt
    achieved_tflops = B * FLOP_PER_SEQ / (enc_ms_avg * 1e-3) / 1e12
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, src_enc, top_s, top_i)

    # ---- parity spot check inside the bench (--full): top-1 ids vs the float64 oracle on a sample
    top1_match = enc_err = None
    if rank == 0 and args.full:
        from oracle import sse_oracle as O
        p = {k: v for k, v in m.get_variables().items()}
        ids_s = src_ids[:48].cpu().numpy()
        want = O.encode(p, params, "src", ids_s)
        tgt_o = O.encode(p, params, "tgt", tgt_ids.cpu().numpy())
        _, wids = O.topk(O.scores_f64(want, tgt_o.astype(np.float64)), 1)
        got = top_i[:48, 0].cpu().numpy()
        top1_match = float(np.mean(got == wids[:, 0]))
        enc_err = float(np.abs(src_enc[:48].cpu().numpy() - want).max())

    # ---- secondary leg: the SAME step with the opt-in split-bf16 encoder (option lstm_x3: three bf16 MFMAs on hi + lo
    # operands per product; ~1e-6 from the exact fp32 kernel).  Not the headline: `value` is the exact fp32 path.
    x3_leg = None
    if not args.no_x3_leg:
        h.set_option("lstm_x3", 1)
        exact_enc = src_enc[:4096].clone()
        for _ in range(max(1, args.warmup)):
            step()
        barrier()
        t0x = time.perf_counter()
        for i in range(args.steps):
            step(i if i < nrec else None)
        barrier()
        dtx = time.perf_counter() - t0x
        h.synchronize()
        if use_dist:
            t = torch.tensor([dtx], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dtx = float(t.item())
        x3_ms = sum(h.timer_elapsed_ms(2 * i, 2 * i + 1) for i in range(nrec)) / nrec
        x3_leg = {"seqs_per_s": world * B * args.steps / dtx, "ms_per_step": dtx / args.steps * 1e3, "encode_kernel_ms": x3_ms,
                  "arithmetic": "v_mfma_f32_32x32x16_bf16 on hi + lo split fp32 operands (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi), fp32 accumulate",
                  "algorithmic_tflops_per_gpu": B * FLOP_PER_SEQ / (x3_ms * 1e-3) / 1e12,
                  "bf16_mfma_tflops_per_gpu": 3 * B * FLOP_PER_SEQ / (x3_ms * 1e-3) / 1e12,
                  "frac_of_bf16_mfma_peak": 3 * B * FLOP_PER_SEQ / (x3_ms * 1e-3) / 1e12 / 2500.0,
                  "max_abs_diff_vs_exact_fp32_kernel": float((src_enc[:4096] - exact_enc).abs().max().item())}
        x3_leg["roofline"] = {"kernel": "lstm_fwd_x3_kernel<8,false,2>", "bound": "mfma", "unit": "TFLOP/s",
                              "achieved": 3 * B * FLOP_PER_SEQ / (x3_ms * 1e-3) / 1e12, "peak": 2500.0,
                              "frac": 3 * B * FLOP_PER_SEQ / (x3_ms * 1e-3) / 1e12 / 2500.0,
                              "note": "executed bf16 MFMA flops = 3 x algorithmic (hi*hi + hi*lo + lo*hi)",
                              "mfma_busy": PMC.get("mfma_busy", {}).get("lstm_fwd_x3_kernel<8, false, 2>")}
        if rank == 0:
            x3_leg["max_abs_err_vs_oracle"] = float(np.abs(src_enc[:48].cpu().numpy() - want).max())
            x3_leg["top1_match_vs_oracle"] = float(np.mean(top_i[:48, 0].cpu().numpy() == wids[:, 0]))
        h.set_option("lstm_x3", 0)

    # ---- secondary leg: mid-size encode batches (the evaluator's 600 rows, sse_evaluator.py:104-109; the index builder's
    # 1000, sse_index.py:66,90-92): the MFMA cluster kernel (lstm_cluster.hip), the exact fp32 chain of the matrix kernel
    mid_leg = None
    if not args.no_x3_leg:
        mid_leg = {"arithmetic": "v_mfma_f32_16x16x4_f32, the matrix kernel's fp32 fma chain (bit-identical results)", "rows": {}}
        for rows in (600, 1024, 2048):
            ref = torch.empty((rows, S), dtype=torch.float32, device=dev)
            h.set_option("lstm_cluster_rows", 0)
            h.set_option("lstm_small_rows", 0)                   # 32-row tiles of the matrix kernel
            h.encode_dev(0, src_ids.data_ptr(), rows, T, True, ref.data_ptr())
            h.set_option("lstm_small_rows", 1024)
            h.set_option("lstm_cluster_rows", 1024)
            for _ in range(3):
                h.encode_dev(0, src_ids.data_ptr(), rows, T, True, src_enc.data_ptr())
            n_it = 20
            for i in range(n_it):
                h.timer_record(2 * i)
                h.encode_dev(0, src_ids.data_ptr(), rows, T, True, src_enc.data_ptr())
                h.timer_record(2 * i + 1)
            h.synchronize()
            ms = sorted(h.timer_elapsed_ms(2 * i, 2 * i + 1) for i in range(n_it))[n_it // 2]
            tf = rows * FLOP_PER_SEQ / (ms * 1e-3) / 1e12
            mid_leg["rows"][str(rows)] = {"encode_ms": ms, "seqs_per_s": rows / (ms * 1e-3), "launches": (rows + 1023) // 1024,
                                          "identical_to_matrix_kernel": bool(torch.equal(src_enc[:rows], ref)),
                                          "roofline": {"kernel": "lstm_cluster_kernel", "bound": "mfma", "unit": "TFLOP/s",
                                                       "achieved": tf, "peak": PEAK_F32_MFMA_TFLOPS, "frac": tf / PEAK_F32_MFMA_TFLOPS}}
        mid_leg["fallbacks"] = h.get_counter("lstm_persist_fallbacks")
        mid_leg["timing"] = "HIP events around the call on the library's stream, median of 20 (device-resident ids and output)"

    # ---- secondary leg: ranking-scale sharded scoring with RCCL all-gather of per-shard top-k
    scoring = None
    shard_bounds = None
    if not args.no_scoring_leg:
        Ns, Q, k = args.score_rows, args.score_queries, 10
        g = torch.Generator(device=dev).manual_seed(7 + rank)
        shard = torch.nn.functional.normalize(torch.randn((Ns, S), generator=g, device=dev), dim=1)
        gq = torch.Generator(device=dev).manual_seed(99)            # identical queries on every rank
        q = torch.nn.functional.normalize(torch.randn((Q, S), generator=gq, device=dev), dim=1)
        noise = torch.randn((Q, S), generator=gq, device=dev)
        mine = torch.arange(Q, device=dev)[torch.arange(Q, device=dev) % world == rank]
        shard[mine] = torch.nn.functional.normalize(q[mine] + 0.1 * noise[mine], dim=1)   # planted: query j -> shard j%world, row j
        sharded = sse_amd.ShardedIndex(h, rank, world, Ns * world, always_gather=force_dist)
        sharded.set_local_rows(shard)
        del shard
        # every rank's [start, end) of the global index, gathered (not recomputed) so that the line shows what each rank used
        if use_dist:
            sb = torch.tensor([sharded.start, sharded.end], dtype=torch.int64, device=dev)
            allsb = [torch.empty_like(sb) for _ in range(world)]
            dist.all_gather(allsb, sb)
            shard_bounds = [[int(x[0]), int(x[1])] for x in allsb]
        else:
            shard_bounds = [[sharded.start, sharded.end]]
        state = {}

        def score_step():
            state["s"], state["i"] = sharded.score_topk(q, k)

        score_step()
        barrier()
        ts = time.perf_counter()
        for _ in range(args.score_iters):
            score_step()
        barrier()
        sdt = (time.perf_counter() - ts) / args.score_iters
        if use_dist:
            t = torch.tensor([sdt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            sdt = float(t.item())
        jj = torch.arange(Q, device=dev)
        planted_ok = float((state["i"][:, 0] == (jj % world) * Ns + jj).double().mean().item())
        # the same pass with fp32 candidates only (option score_bf16 = 0): the library default selects candidates on the
        # bf16 matrix pipe and re-scores in float64 with the bound widened to the bf16 rounding -- ids and scores must be
        # bit-identical between the two, checked here on every run
        ref_s, ref_i = state["s"].clone(), state["i"].clone()
        h.set_option("score_bf16", 0)
        score_step()
        barrier()
        ts = time.perf_counter()
        for _ in range(args.score_iters):
            score_step()
        barrier()
        fdt = (time.perf_counter() - ts) / args.score_iters
        h.set_option("score_bf16", 1)
        if use_dist:
            t = torch.tensor([fdt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            fdt = float(t.item())
        same = bool(torch.equal(state["i"], ref_i) and torch.equal(state["s"], ref_s))
        scoring_fp32 = {"scores_per_s": Q * Ns * world / fdt, "ms_per_pass": fdt * 1e3,
                        "achieved_tflops_per_gpu": 2.0 * S * Q * Ns / fdt / 1e12,
                        "frac_of_f32_mfma_peak": 2.0 * S * Q * Ns / fdt / 1e12 / PEAK_F32_MFMA_TFLOPS,
                        "identical_to_default": same,
                        "roofline": {"kernel": "score_topk_kernel<4,false,false,true>", "bound": "mfma", "unit": "TFLOP/s",
                                     "achieved": 2.0 * S * Q * Ns / fdt / 1e12, "peak": PEAK_F32_MFMA_TFLOPS,
                                     "frac": 2.0 * S * Q * Ns / fdt / 1e12 / PEAK_F32_MFMA_TFLOPS,
                                     "note": "whole pass (sweep + float64 re-scoring + follow-up launches) over the sweep's algorithmic flops",
                                     "mfma_busy": PMC.get("mfma_busy", {}).get("score_topk_kernel<4, false, false, true>")}}
        scoring = {"scores_per_s": Q * Ns * world / sdt, "ms_per_pass": sdt * 1e3, "queries": Q,
                   "index_rows_total": Ns * world, "index_rows_per_gpu": Ns, "S": S, "k": k,
                   "collective": "rccl all_gather of per-shard top-k + k-way merge" if world > 1 else "none (1 shard)",
                   "candidates": "bf16 MFMA (v_mfma_f32_32x32x16_bf16) + exact float64 re-scoring, fp32 second chance on the device",
                   "algorithmic_tflops_per_gpu": 2.0 * S * Q * Ns / sdt / 1e12,
                   "top1_planted_acc": planted_ok, "identical_to_fp32_candidates": same,
                   "roofline": {"kernel": "score_topk_kernel<4,true,false,true>", "bound": "mfma", "unit": "TFLOP/s",
                                "achieved": 2.0 * S * Q * Ns / sdt / 1e12, "peak": 2500.0, "frac": 2.0 * S * Q * Ns / sdt / 1e12 / 2500.0,
                                "note": "whole pass (bf16 sweep + float64 re-scoring + second-chance / collect launches) over the "
                                        "sweep's algorithmic flops; peak = the 2.5 PF datasheet figure; a register-only "
                                        "v_mfma_f32_32x32x16_bf16 loop on random data sustains 1.70 PF on this part at "
                                        "1.71 GHz (tools/mfma_peak_bf16.hip, profiles/r04_notes.txt)",
                                "sustained_mfma_tflops_measured": 1700.0,
                                "frac_of_sustained": 2.0 * S * Q * Ns / sdt / 1e12 / 1700.0,
                                "mfma_busy": PMC.get("mfma_busy", {}).get("score_topk_kernel<4, true, false, true>")}}

    # ---- secondary leg: the demo / web path (sse_demo.py:112-134, webserver.py:124-161): ONE query, token ids in ->
    # top-10 out, against the 571-row classification index and against this rank's ranking shard.  The big sweep is
    # HBM-bound: algorithmic bytes = rows * S * 2 (the bf16 candidate copy of the index is streamed once).
    latency = None
    if rank == 0 and not args.no_scoring_leg:
        one = src_ids[:1].cpu().numpy()
        def timed(fn, n=31):
            # median of per-call times (one call in a few thousand stalls for tens of ms inside the HIP runtime with the
            # GPU idle: a mean over 20 calls turns that into +1.7 ms on every call, profiles/r03_notes.txt)
            fn()
            ts = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return sorted(ts)[n // 2]
        h.index_set_dev(tgt_enc.data_ptr(), N_TARGETS, S)
        # the cluster kernels are launched cooperatively by default (co-residency guaranteed by the runtime); the plain
        # launch (option lstm_cluster_coop = 0) is ~20 us quicker per call: both are reported
        h.set_option("lstm_cluster_coop", 0)
        e2e_small_plain = timed(lambda: h.encode_score_topk(0, one, False, 10))
        enc_only_plain = timed(lambda: h.encode(0, one, False))
        h.set_option("lstm_cluster_coop", 1)
        e2e_small = timed(lambda: h.encode_score_topk(0, one, False, 10))
        enc_only = timed(lambda: h.encode(0, one, False))
        qd = src_enc[:1].contiguous()
        os1 = torch.empty((1, 10), dtype=torch.float64, device=dev)
        oi1 = torch.empty((1, 10), dtype=torch.int64, device=dev)
        Ns = args.score_rows
        g = torch.Generator(device=dev).manual_seed(7)
        big = torch.nn.functional.normalize(torch.randn((Ns, S), generator=g, device=dev), dim=1)
        h.index_set_dev(big.data_ptr(), Ns, S)
        del big
        e2e_big = timed(lambda: h.encode_score_topk(0, one, False, 10))
        def sweep():
            h.score_topk_dev(qd.data_ptr(), 1, 10, os1.data_ptr(), oi1.data_ptr())
            torch.cuda.synchronize()
        sweep_s = timed(sweep)
        latency = {"query": "1 dense sequence, T=%d (no padding: worst case)" % T,
                   "encode_ms": enc_only * 1e3, "ids_to_top10_ms_index_571": e2e_small * 1e3,
                   "encode_ms_plain_launch": enc_only_plain * 1e3, "ids_to_top10_ms_index_571_plain_launch": e2e_small_plain * 1e3,
                   "ids_to_top10_ms_index_%d" % Ns: e2e_big * 1e3, "sweep_ms_index_%d" % Ns: sweep_s * 1e3,
                   "sweep_hbm": {"bound": "hbm", "algorithmic_bytes": Ns * S * 2, "achieved_gbps": Ns * S * 2 / sweep_s / 1e9,
                                 "peak_gbps": 8000.0, "hbm_frac": Ns * S * 2 / sweep_s / 8e12},
                   "roofline": {"kernel": "score_topk_kernel<1,true,false,true> (+ re-scoring, one synchronisation)", "bound": "hbm",
                                "unit": "GB/s", "achieved": Ns * S * 2 / sweep_s / 1e9, "peak": 8000.0,
                                "frac": Ns * S * 2 / sweep_s / 8e12,
                                "traffic": PMC.get("sweep_q1_hbm_bytes"),
                                "note": "algorithmic bytes = the bf16 candidate copy of the index streamed once; the call also "
                                        "holds the pack / re-score launches and the host round trip"},
                   "timing": "median of 31 calls",
                   "note": "host buffers both ways (ids H2D, top-10 D2H, one synchronisation)"}
        h.index_set_dev(tgt_enc.data_ptr(), N_TARGETS, S)

    # ---- secondary leg: data-parallel train step (fwd + loss + BPTT, ONE flat RCCL all-reduce, clip + Adagrad);
    # runs last because it updates the weights
    training = None
    if not args.no_train_leg:
        rng = np.random.RandomState(1234 + rank)
        Bt = args.train_rows
        tsrc = np.repeat(rng.randint(2, V, size=(Bt // 2, T)).astype(np.int32), 2, axis=0)   # data.py:95-115: pos,neg share a source
        ttgt = rng.randint(2, V, size=(Bt, T)).astype(np.int32)
        tsrc[:, -1] = 1
        ttgt[:, -1] = 1
        tz = np.tile(np.array([1.0, 0.0], np.float32), Bt // 2)
        trainer = sse_amd.DataParallelTrainer(h, device=dev, always_reduce=force_dist)
        # the (synthetic) corpora are resident on the device, as in sse_train: a step ships 2 x Bt row numbers
        h.corpus_upload(0, tsrc[0::2])
        h.corpus_upload(1, ttgt)
        src_rows = np.repeat(np.arange(Bt // 2, dtype=np.int32), 2)          # data.py:95-115: pos,neg share a source
        tgt_rows = np.arange(Bt, dtype=np.int32)
        def timed_steps():
            t = trainer.train_step(src_rows, tgt_rows, tz, rows_global=Bt * world, by_rows=True)
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.train_iters):
                t = trainer.train_step(src_rows, tgt_rows, tz, rows_global=Bt * world, by_rows=True)
            barrier()
            d = (time.perf_counter() - t0) / args.train_iters
            if use_dist:
                tt = torch.tensor([d], dtype=torch.float64, device=dev)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                d = float(tt.item())
            return d, t
        # the opt-in split-bf16 arithmetic first, then the library default = exact fp32 (the reference's arithmetic): the
        # default is `ms_per_step` and the roofline below
        for opt in ("train_dk_x3", "train_fwd_x3", "train_bwd_x3"):
            h.set_option(opt, 1)
        xdt_train, _ = timed_steps()
        for opt in ("train_fwd_x3", "train_bwd_x3", "train_dk_x3"):
            h.set_option(opt, 0)
        tdt, tl = timed_steps()
        # fp32 MFMA flops the default step EXECUTES per GPU (paired batch: the source encoder's forward and weight-gradient GEMM
        # run once per (pos, neg) pair): forward gates + projection, BPTT recurrence dG.Kh^T, dX = dG.Kx^T, dK = A^T dG
        fwd = (Bt + Bt // 2) * FLOP_PER_SEQ
        rec = 2 * Bt * T * 2 * H * 4 * H
        dxf = 2 * Bt * T * 2 * 4 * H * E
        dkf = (Bt + Bt // 2) * T * 2 * (E + H) * 4 * H
        executed = float(fwd + rec + dxf + dkf)
        training = {"pair_rows_per_s": Bt * world / tdt, "ms_per_step": tdt * 1e3, "pair_rows_per_gpu": Bt,
                    "ms_per_step_split_bf16_opt_in": xdt_train * 1e3,
                    "collective": ("rccl all_reduce of one flat %.1f MB gradient buffer" % (trainer.arena.numel() * 4 / 1e6))
                    if world > 1 else "none (1 rank)",
                    "algorithmic_tflops_per_gpu": 3.0 * 2 * Bt * FLOP_PER_SEQ / tdt / 1e12,
                    "algorithmic_note": "SURVEY 8d: train ~ 3 x forward flops for both encoders, no pair de-duplication (not a roofline figure)",
                    "loss_last": tl[0], "input": "corpus resident on the device; 2 x %d int32 row numbers H2D per step" % Bt,
                    "arithmetic": "fp32 throughout (library default since round 4 = the reference's tf.float32): forward, BPTT "
                                  "(recurrence + dX) and weight-gradient GEMMs on v_mfma_f32_32x32x2_f32; projections, loss, clip and "
                                  "Adagrad in fp32.  ms_per_step_split_bf16_opt_in = options train_fwd_x3 / train_bwd_x3 / train_dk_x3 "
                                  "= 1 (three bf16 MFMAs on hi + lo split operands per product, ~4e-6 relative)",
                    "roofline": {"kernel": "whole step: lstm_fwd_kernel<TRAIN, tape_swap> x2, lstm_bwd2_kernel x2 (+ dx_scatter), dk_gemm3 / dk_gemm2 (paired side)", "bound": "mfma",
                                 "unit": "TFLOP/s", "achieved": executed / tdt / 1e12, "peak": PEAK_F32_MFMA_TFLOPS,
                                 "frac": executed / tdt / 1e12 / PEAK_F32_MFMA_TFLOPS,
                                 "executed_mfma_flop_per_step": executed,
                                 "note": "whole step over the fp32 MFMA flops it executes (with pair de-duplication)",
                                 "mfma_busy": busy_of("lstm_bwd", "void lstm_bwd", "dk_gemm", "void dk_gemm", "lstm_fwd_kernel<2, 2, 1, true", "void lstm_fwd_kernel<2, 2, 1, true", "lstm_fwd_kernel<1, 1, 1, true", "void lstm_fwd_kernel<1, 1, 1, true")}}

    # ---- secondary legs on their own models: the reference's recipe shapes, and the text-CNN of configs[4]
    shapes_leg = reference_shapes_leg(sse_amd, torch, dev) if (rank == 0 and not args.no_shapes_leg) else None
    cnn = cnn_leg(sse_amd, torch, np, dev) if (rank == 0 and not args.no_cnn_leg) else None
    realdata = realdata_leg(sse_amd, torch, np, dev) if (rank == 0 and world == 1 and not args.no_realdata_leg) else None
    sweep = None
    if rank == 0 and world == 1 and not args.no_sweep_leg:
        m_sw = sse_amd.SSEModel(params, device=local_rank)      # (the main model's weights were updated by the train leg)
        m_sw.init_variables(seed=0)
        sweep = config_sweep_leg(sse_amd, torch, dev, m_sw.handle)
        m_sw.handle.close()
    barrier()

    traffic = PMC.get("lstm_fwd_hbm_bytes_per_launch") if B == 16384 else None   # PMC pass of this same command, same sources
    if rank == 0:
        line = {
            "metric": "encoded seqs/sec (+ query x target cosine-scores/sec, top-1 vs ref)",
            "value": value, "unit": "seqs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[1]: classification stand-in, dual-encoder LSTM H=S=256 E=50 T=32 "
                                   "V=32000; encode %d source seqs/GPU/step + cosine top-10 vs 571-target index" % B,
                       "batch_per_gpu": B, "seq_len": T, "targets": N_TARGETS, "parallelism": "dp%d" % world,
                       "weights": "random-init (reference initialisers, seed 0)"},
            "cosine_scores_per_s": value * N_TARGETS,
            "roofline": {"kernel": "lstm_fwd_kernel<2>", "bound": "mfma", "achieved": achieved_tflops,
                         "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": achieved_tflops / PEAK_F32_MFMA_TFLOPS,
                         "traffic": traffic, "traffic_unit": "bytes/launch (PMC: (2 x FETCH_SIZE + WRITE_SIZE) x 1024, separate rocprofv3 "
                                                             "passes of this command; null when the kernel sources changed since)",
                         "mfma_busy": (busy_of("lstm_fwd_kernel<2, 2, 1, false, true") or {None: None}).popitem()[1],
                         "pmc_source": PMC.get("source", PMC.get("stale")),
                         "traffic_measured_in_this_run": False,
                         "pmc_note": "traffic / mfma_busy (here and in every leg) are REPLAYED from the tracked profiles/pmc_summary.json -- the "
                                     "builder's separate rocprofv3 --pmc passes of this same command, quoted only while the hash of csrc/ "
                                     "matches -- they are not counted in this run; achieved / avg_kernel_ms ARE measured in this run (HIP events)",
                         "avg_kernel_ms": enc_ms_avg,
                         "algorithmic_flop_per_launch": B * FLOP_PER_SEQ},
        }
        if args.full:
            line.update({"rccl_ranks_seen": rccl_ranks_seen, "shard_bounds": shard_bounds,
                         "top1_match_vs_oracle": top1_match, "encode_max_abs_err_vs_oracle": enc_err})
        if scoring is not None:
            line["scoring_leg"] = scoring
            line["scoring_leg_fp32_candidates"] = scoring_fp32
        if x3_leg is not None:
            line["encode_leg_split_bf16"] = x3_leg
        if mid_leg is not None:
            line["encode_leg_mid_batch"] = mid_leg
        if latency is not None:
            line["latency_leg"] = latency
        if training is not None:
            line["train_leg"] = training
        if shapes_leg is not None:
            line["encode_leg_reference_shapes"] = shapes_leg
        if cnn is not None:
            line["cnn_leg"] = cnn
        if realdata is not None:
            line["realdata_leg"] = realdata
        if sweep is not None:
            line["config_sweep"] = sweep
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline()
            line["speedup_vs_cpu_baseline"] = value / line["cpu_baseline"]["value"]
        emit(line, with_legs=args.full)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    if len(sys.argv) >= 6 and sys.argv[1] == "--cpu-worker":
        cpu_replica_worker(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), float(sys.argv[5]))
    else:
        main()
