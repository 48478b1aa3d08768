#!/bin/bash
# Every GPU test and smoke on the tree as committed, then the C5 and C3 benches with everything they
# measure (--full).  Logs go to $OUT (default: bench_out/ in the repository).
# Usage: tools/gpu_final_check.sh <tag>
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/bench_out}
cd "$ROOT" && mkdir -p "$OUT"
tag=${1:-fin}
timeout -k 10 700 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread -rfs \
  > "$OUT/${tag}_pytest_gpu.log" 2>&1 || exit $?
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/${tag}_smoke.log" 2>&1 || exit $?
timeout -k 10 600 python bench.py --full --config c5 --no-cpu-baseline > "$OUT/${tag}_bench_c5.log" 2>&1 || exit $?
timeout -k 10 300 python bench.py --full > "$OUT/${tag}_bench.log" 2>&1
