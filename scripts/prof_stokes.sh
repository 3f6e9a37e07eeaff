#!/bin/bash
# kernel-level profile of the Stokes-control workload (launches instead of graphs)
set -e
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp KKT_NO_GRAPH=1
out=${1:?usage: prof_stokes.sh OUTPUT_DIR}
mkdir -p "$out"
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$out" -o st --output-format csv -- python3 bench.py --full --workload stokes2d --steps 3 --warmup 1 > "$out/bench.json" 2> "$out/bench.err"
ls -R "$out" | head -20
