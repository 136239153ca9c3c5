#!/bin/bash
# One GPU-box session: parity tests, then the bench (and optional extra steps).
# Each GPU step runs under its own time limit; a fault, abort, segfault or
# time limit (124/134/137/139) ends the script; an ordinary test failure
# (exit 1) still lets the bench run so its numbers come back.
#   bash tools/gpu_run.sh [pytest-args...]
OUT=${OUT:-bench_out}  # results go here (relative to the repo root)
mkdir -p "$OUT"
fatal() { case "$1" in 124|134|137|139) return 0 ;; *) return 1 ;; esac; }

timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread "$@" \
  > $OUT/pytest.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -5 $OUT/pytest.log
if fatal $rc; then exit $rc; fi

timeout -k 10 300 python -u bench.py --full --steps 20 --warmup 3 > $OUT/bench.json 2> $OUT/bench.err
rc=$?
echo "bench rc=$rc"; cat $OUT/bench.json; tail -3 $OUT/bench.err
if fatal $rc; then exit $rc; fi

timeout -k 10 300 python -u bench.py --full --steps 20 --warmup 3 --cpu-seconds 0 --overlap 0 > $OUT/bench_no_overlap.json \
  2> $OUT/bench_no_overlap.err
rc=$?
echo "bench (one stream) rc=$rc"; cat $OUT/bench_no_overlap.json
if fatal $rc; then exit $rc; fi

timeout -k 10 300 python -u bench.py --workload server --steps 5 --warmup 2 > $OUT/bench_server.json \
  2> $OUT/bench_server.err
rc=$?
echo "bench server rc=$rc"; cat $OUT/bench_server.json; tail -3 $OUT/bench_server.err
if fatal $rc; then exit $rc; fi

timeout -k 10 300 python -u bench.py --workload server --steps 5 --warmup 2 --request 1 > $OUT/bench_server_shuffled.json \
  2> $OUT/bench_server_shuffled.err
rc=$?
echo "bench server (per-message shuffle) rc=$rc"; cat $OUT/bench_server_shuffled.json
if fatal $rc; then exit $rc; fi

timeout -k 10 300 python -u bench.py --workload server --steps 5 --warmup 2 --zipf 1.2 > $OUT/bench_server_zipf.json \
  2> $OUT/bench_server_zipf.err
rc=$?
echo "bench server (config 5, Zipf owners) rc=$rc"; cat $OUT/bench_server_zipf.json; tail -3 $OUT/bench_server_zipf.err
exit $rc
