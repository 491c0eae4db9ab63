#!/bin/bash
# rocprofv3 kernel stats of the full bench (secondary legs, no CPU baseline, no train leg).
# usage (repo root): bash tools/prof_bench_quick.sh <output dir>
root=$(pwd); out=$(realpath -m "${1:?usage: tools/prof_bench_quick.sh <output dir>}"); mkdir -p "$out"; export TMPDIR=/tmp; cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/pb" -o p -- python "$root/bench.py" --full --no-cpu-baseline --no-train-leg > "$out/pb.log" 2>&1
tail -1 "$out/pb.log" | cut -c1-220
grep -E "rescore|score_topk|lstm_fwd_kernel<2" "$out/pb/p_kernel_stats.csv" | cut -c1-130
