#!/bin/bash
# GPU parity tests, then a short bench (the iteration loop of a round).
# usage: [BENCH_OUT=dir] tools/gpu_check.sh [bench args...]   (on the GPU box, from the repo root)
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$R"
OUT=${BENCH_OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1
rc=$?
tail -3 "$OUT/gpu_tests.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python3 bench.py --full --no-cpu-baseline "$@" > "$OUT/bench.json" 2> "$OUT/bench.err"
rc=$?
cat "$OUT/bench.json"
exit $rc
