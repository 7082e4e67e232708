#!/bin/bash
# One GPU round on the MI355X box (run from the repo root via gpurun):
# GPU parity tests, the bench line, a kernel-trace profile of the same bench
# command (one batch in flight, as the bench's kernel timers run) and the PMC
# passes.  Outputs under $OUT/.  Any failing step ends the script.
set -e
OUT=${OUT:-bench_out}  # outputs go here, relative to the repository root
R=$GRAFT_REPO_ROOT
TAG=${1:-latest}
mkdir -p $R/$OUT
cd $R
if [ "${OTM_TESTS:-1}" = "1" ]; then
  timeout -k 10 700 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
fi
timeout -k 10 400 python -u bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err
(cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/prof1 -o run -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-check --host-steps 0 --json-calls 0 --inflight 1 > $R/$OUT/prof1.log 2>&1)
if [ "${OTM_PMC:-1}" = "1" ]; then PMC_STATS_CSV=$R/$OUT/prof1/run_kernel_stats.csv bash scripts/pmc.sh $OUT/pmc $TAG; fi
