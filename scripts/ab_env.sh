#!/bin/bash
# A/B of one env knob over short bench runs: bash scripts/ab_env.sh VAR v1 v2 ...
set -e
OUT=${OUT:-bench_out}  # outputs go here, relative to the repository root
VAR=$1; shift
mkdir -p $OUT/ab
for v in "$@"; do
  env $VAR=$v timeout -k 10 120 python -u bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-check > $OUT/ab/$VAR.$v.json 2> $OUT/ab/$VAR.$v.err
done
