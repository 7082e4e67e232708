#!/bin/bash
# Secondary bench lines (configs 3 and 4) with config 4's kernel trace and
# PMC passes.  GPU box, repo root: bash scripts/gpu_configs.sh <tag>
set -e
OUT=${OUT:-bench_out}  # outputs go here, relative to the repository root
R=$GRAFT_REPO_ROOT
TAG=${1:-latest}
mkdir -p $R/$OUT
cd $R
timeout -k 10 400 python -u bench.py --full --config 3 --steps 5 --warmup 2 > $OUT/bench_c3.json 2> $OUT/bench_c3.err
(cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/prof_c4 -o run -- python3 $R/bench.py --full --config 4 --steps 5 --warmup 2 --no-cpu-baseline --no-check --inflight 1 > $R/$OUT/prof_c4.log 2>&1)
PMC_BENCH_ARGS="--config 4" PMC_STATS_CSV=$R/$OUT/prof_c4/run_kernel_stats.csv bash scripts/pmc.sh $OUT/pmc_c4 c4_$TAG
timeout -k 10 400 python -u bench.py --full --config 4 --steps 5 --warmup 2 --traffic-json $OUT/pmc_c4/pmc_traffic_c4_$TAG.json > $OUT/bench_c4.json 2> $OUT/bench_c4.err
