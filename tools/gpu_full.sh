#!/bin/bash
# The whole GPU suite (one process, per-test time limit) and the default
# bench line, as the driver runs them at round end.
export PYTHONUNBUFFERED=1
OUT=${OUT:-bench_out}  # results go here (relative to the repo root)
mkdir -p "$OUT"
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
  > $OUT/pytest_full.log 2>&1
rc=$?
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
timeout -k 10 600 python -u bench.py --full > $OUT/bench_full.json 2> $OUT/bench_full.err
