#!/bin/bash
# the whole bench (headline, roofline, CPU baseline, secondaries): bash tools/gpu_bench_full.sh <output dir>
O=${1:?usage: $0 <output dir>}
mkdir -p "$O"
timeout -k 10 1000 python bench.py --full > "$O/bench_full.json" 2> "$O/bench_full.err"; echo "bench rc $?"
tail -3 "$O/bench_full.err"
python tools/bench_summary.py "$O/bench_full.json"
