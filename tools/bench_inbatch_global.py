#!/usr/bin/env python
"""Timing of the in-batch softmax loss over the global batch of a data-parallel step.  Writes profiles/inbatch_global.txt (or --out).

    python tools/bench_inbatch_global.py [--parent-lib /path/to/the/parent/commit's/libsse_hip.so]

Head: sse_inbatch_loss_window_dev at global B in {1024, 8192} x S 256 with a window of B / 8 rows (what one of eight ranks runs;
the window in the middle of the batch), beside sse_inbatch_loss_dev on the same inputs on this build and -- with --parent-lib --
on the parent's build.  Random encodings, every row distinct, half the labels 1; median (smallest .. largest) of REPS timed
batches of back-to-back calls between two HIP events, after WARM untimed calls.
Step: one rank in a 1-rank `nccl` group, DataParallelTrainer(always_reduce=True) at 1024 pair rows, V 32000, E 50, H = S = 256,
T 32, option train_loss = 1: global_negatives=True on this build against the plain train_loss = 1 step (the rank's own rows) on
this build and on the parent's, the latter also with option train_pair_dedup = 0 (an open step never de-duplicates pairs).
Wall time of the synchronous train_step, median of STEP_REPS steps after STEP_WARM.
Every measurement runs in a child process of its own, RUNS times, alternating between the builds (DESIGN K6); the table shows
the median of the runs' medians and their smallest and largest: the spread between runs is the noise floor a difference has to
exceed."""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 7
STEP_WARM, STEP_REPS = 5, 30
RUNS = 5
HEAD_SHAPES = ((1024, 256), (8192, 256))
CHILD_LIMIT_S = 240


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def load():
    """sse_amd on the library SSE_HIP_LIB names; entry points that build lacks (the parent's) leave the symbol table first."""
    import sse_amd
    path = os.environ.get("SSE_HIP_LIB")
    if path:
        lib = ctypes.CDLL(path)
        for n in [n for n in sse_amd.SYMBOLS if not hasattr(lib, n)]:
            del sse_amd.SYMBOLS[n]
    return sse_amd


def time_calls(call, calls):
    import torch
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
    return median(out)


def measure_heads(sse_amd, res):
    import torch
    from tests.util import model_params
    h = sse_amd.SSEModel(model_params("dual-encoder", V=20, E=8, Hs=16, Ht=16, S=8, T=4)).handle
    dev = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    for B, S in HEAD_SHAPES:
        g = torch.Generator(device=dev).manual_seed(B * 1000 + S)
        s = torch.randn(B, S, device=dev, generator=g)
        t = 0.3 * s + torch.randn(B, S, device=dev, generator=g)
        z = (torch.arange(B, device=dev) % 2 == 0).float()
        ds, dt, rl, ra = torch.empty(B, S, device=dev), torch.empty(B, S, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
        calls = 20 if B <= 1024 else 3
        res["head_full_%d_%d" % (B, S)] = time_calls(lambda: h.inbatch_loss_dev(s, t, z, None, None, B, S, 64.0, 1.0 / B, ds, dt, rl, ra, st), calls)
        if "sse_inbatch_loss_window_dev" in sse_amd.SYMBOLS:
            W = B // 8
            lo = 3 * W
            res["head_window_%d_%d" % (B, S)] = time_calls(
                lambda: h.inbatch_loss_window_dev(s, t, z, None, None, B, S, lo, lo + W, 64.0, 1.0 / B, ds, dt, rl, ra, st), calls)
            res["head_window_whole_%d_%d" % (B, S)] = time_calls(
                lambda: h.inbatch_loss_window_dev(s, t, z, None, None, B, S, 0, B, 64.0, 1.0 / B, ds, dt, rl, ra, st), calls)


def measure_steps(sse_amd, res):
    import torch
    import torch.distributed as dist
    from tests.util import model_params
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
    sock.close()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    B, V, T = 1024, 32000, 32
    params = model_params("dual-encoder", V, 50, 256, 256, 256, T, lr=0.05)
    rng = np.random.RandomState(0)
    src = np.repeat(rng.randint(2, V, size=(B // 2, T)).astype(np.int32), 2, axis=0)
    tgt = rng.randint(2, V, size=(B, T)).astype(np.int32)
    z = np.tile(np.array([1.0, 0.0], np.float32), B // 2)
    # (the batch is paired and 1024 % 128 == 0: the plain step runs its source encoder on one row of every pair, option
    # train_pair_dedup, which an open step does not; step_local_nodedup is the plain step without it, for the attribution)
    kinds = [("step_local", False, 1), ("step_local_nodedup", False, 0)]
    if "sse_train_forward" in sse_amd.SYMBOLS:
        kinds.append(("step_global", True, 1))
    for name, global_negatives, dedup in kinds:
        m = sse_amd.SSEModel(params)
        m.init_variables(seed=1)
        m.handle.set_option("train_pair_dedup", dedup)
        kw = dict(global_negatives=True) if global_negatives else {}
        tr = sse_amd.DataParallelTrainer(m.handle, device="cuda:0", always_reduce=True, options={"train_loss": 1, "train_loss_scale": 64}, **kw)
        ms = []
        for i in range(STEP_WARM + STEP_REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train_step(src, tgt, z, rows_global=B)
            torch.cuda.synchronize()
            if i >= STEP_WARM:
                ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = median(ms)
        res[name + "_paired_steps"] = m.handle.get_counter("train_paired_steps")
        m.handle.set_stream(0)
        m.handle.close()
    dist.destroy_process_group()


def child():
    import torch
    torch.cuda.set_device(0)            # torch's HIP runtime first: the library then shares it
    torch.cuda.current_stream()
    sse_amd = load()
    res = {}
    measure_heads(sse_amd, res)
    measure_steps(sse_amd, res)
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib):
    env = dict(os.environ)
    env.pop("SSE_HIP_LIB", None)
    if lib:
        env["SSE_HIP_LIB"] = lib
    out = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child"], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL, text=True, cwd=ROOT)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("a measurement process ended with code %d: nothing more is started" % out.returncode)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def fmt(runs, key):
    xs = [r[key] for r in runs if key in r]
    if not xs:
        return "%-34s -" % key
    return "%-34s %9.4f ms   (runs %.4f .. %.4f)" % (key, median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libsse_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbatch_global.txt"))
    a = ap.parse_args()
    if a.child:
        return child()
    new, parent = [], []
    for _ in range(RUNS):                                     # alternating, one process per measurement
        new.append(run_child(None))
        if a.parent_lib:
            parent.append(run_child(os.path.abspath(a.parent_lib)))
        print("run %d of %d done" % (len(new), RUNS), flush=True)
    lines = ["in-batch softmax loss over the global batch (tools/bench_inbatch_global.py): %d alternating runs per build, a process each;" % RUNS,
             "median of the runs' medians, smallest and largest run beside it", ""]
    for title, runs in (("this build", new), ("parent build", parent)):
        if not runs:
            continue
        lines.append("== %s" % title)
        for B, S in HEAD_SHAPES:
            for k in ("head_full_%d_%d", "head_window_%d_%d", "head_window_whole_%d_%d"):
                if any(k % (B, S) in r for r in runs):
                    lines.append(fmt(runs, k % (B, S)))
        for k in ("step_local", "step_local_nodedup", "step_global"):
            if any(k in r for r in runs):
                lines.append(fmt(runs, k))
        lines.append("paired steps counted: local %s, global %s" % (runs[0].get("step_local_paired_steps"), runs[0].get("step_global_paired_steps")))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
