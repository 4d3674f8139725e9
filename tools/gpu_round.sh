#!/bin/bash
# One GPU-box session: parity tests, smoke, short bench with its sub-benches (--full).
# Stops at the first GPU fault, abort or timeout (exit codes other than 0/1).
# Logs go to $MLGATE_OUT (default: out/).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${MLGATE_OUT:-out}"
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -v -rf --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1
rc=$?; echo "pytest rc=$rc"; tail -25 "$OUT/pytest_gpu.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
rc=$?; echo "smoke rc=$rc"; tail -5 "$OUT/smoke.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python bench.py ${BENCH_ARGS:---full --steps 3 --warmup 1} > "$OUT/bench.log" 2>&1
rc=$?; echo "bench rc=$rc"; tail -5 "$OUT/bench.log"
exit $rc
