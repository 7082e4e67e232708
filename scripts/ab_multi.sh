#!/bin/bash
# Short bench runs under several env settings: bash scripts/ab_multi.sh "A=1 B=2" "A=3" ...
set -e
OUT=${OUT:-bench_out}  # outputs go here, relative to the repository root
mkdir -p $OUT/ab
i=0
for setting in "$@"; do
  env $setting timeout -k 10 120 python -u bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-check > $OUT/ab/run$i.json 2> $OUT/ab/run$i.err
  echo "$setting" > $OUT/ab/run$i.env
  i=$((i+1))
done
