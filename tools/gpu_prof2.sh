#!/bin/bash
# Round-2 profiles: kernel trace + stats of the default bench line, and the two
# HBM traffic PMC passes (separate runs, --pmc only), each under its own limit.
R=$(pwd)
OUT=${OUT:-bench_out}  # results go here (relative to the repo root)
mkdir -p "$R/$OUT"
cd /tmp && export TMPDIR=/tmp
set -e
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/prof" -o run -- \
  python3 "$R/bench.py" --full --steps 20 --warmup 3 --cpu-seconds 0 > "$R/$OUT/prof_bench.json"
B=(python3 "$R/bench.py" --full --steps 3 --warmup 1 --cpu-seconds 0)
timeout -s KILL 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$R/$OUT/pmc_fetch" -o run -- "${B[@]}" > /dev/null
timeout -s KILL 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$R/$OUT/pmc_write" -o run -- "${B[@]}" > /dev/null
cd "$R"
python3 tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write > $OUT/traffic.json
echo prof done
