#!/bin/bash
# Runs bench.py's headline workload (and its roofline pass) against every library under
# aura_snn_rag_amd/lib/variants/: bash tools/variant_sweep.sh <output dir>
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${1:?usage: $0 <output dir>}" && cd "$1" && pwd)
cd /tmp && export TMPDIR=/tmp
for so in $ROOT/aura_snn_rag_amd/lib/variants/libaura_*.so; do
  n=$(basename $so .so)
  AURA_HIP_LIB=$so timeout -k 10 200 python3 $ROOT/bench.py --full --no-secondary --no-cpu-baseline --steps ${STEPS:-200} > $OUT/variant_$n.json 2> $OUT/variant_$n.err || { tail -5 $OUT/variant_$n.err; exit 1; }
  python3 -c "
import json; d=json.load(open('$OUT/variant_$n.json'))
print('$n', 'ms/step', round(d['ms_per_step'],4), 'filter kernel_ms', round(d['roofline']['avg_kernel_ms'],4), 'frac', round(d['roofline']['frac'],3))
"
done
