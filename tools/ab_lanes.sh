#!/bin/bash
# Tail lanes A/B on the default bench (GPU box): bash tools/ab_lanes.sh [OUTDIR]
set -o pipefail
OUT=${1:-$(mktemp -d)}
mkdir -p $OUT
for L in 2 4 3; do
  timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --no-configs --steps 3 --warmup 1 --lanes $L > $OUT/lanes_$L.json 2> $OUT/lanes_$L.err || { tail $OUT/lanes_$L.err; exit 1; }
  python3 -c "import json;d=json.load(open('$OUT/lanes_$L.json'));print('lanes', $L, d['ms_per_step'], d['roofline']['phase_s'])"
done
