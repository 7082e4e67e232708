#!/bin/bash
# GPU tests, then the bench at 3 (default), 1 and 4 batches in flight.
# Run from the repository root; outputs under $OUT/.
set -e
OUT=${OUT:-bench_out}  # outputs go here, relative to the repository root
mkdir -p $OUT
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > $OUT/bench3.json 2> $OUT/bench3.err
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --no-check --inflight 1 > $OUT/bench1.json 2>> $OUT/bench3.err
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --no-check --inflight 4 > $OUT/bench4.json 2>> $OUT/bench3.err
