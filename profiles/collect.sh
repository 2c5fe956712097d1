#!/bin/bash
# Round profile collection on the GPU box (run from the repo root):
#   1. rocprofv3 --kernel-trace --stats of the default bench with its profile leg (graph-replayed
#      steps + the serial per-op profile pass bench.py --full uses for its roofline) -> $OUT/prof_$R/
#   2. two PMC passes (FETCH_SIZE, WRITE_SIZE: they cannot share a pass) of a short bench
# then summarise into profiles/ with kernel_trace_summary.py / pmc_traffic.py (on the CPU side).
#   bash profiles/collect.sh [round tag] [output folder, default profile_out]
set -e
R=${1:-r2}
OUT=${2:-profile_out}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$R -o run -- \
  python3 bench.py --steps 10 --warmup 3 --full --no-cpu --breakdown $OUT/breakdown_$R.json \
  > $OUT/bench_prof_$R.log 2>&1
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmcf_$R -o run -- \
  python3 bench.py --steps 2 --warmup 1 --full --no-cpu > $OUT/pmcf_$R.log 2>&1
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmcw_$R -o run -- \
  python3 bench.py --steps 2 --warmup 1 --full --no-cpu > $OUT/pmcw_$R.log 2>&1
