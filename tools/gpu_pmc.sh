#!/bin/bash
# PMC passes over the C3 bench at one batch in flight (rocprofv3 PMC slots on gfx950):
# FETCH_SIZE and WRITE_SIZE each need a pass of their own (TCC slots); the compute pass
# takes rocprofv3's derived MfmaUtil / VALUBusy / VALUUtilization and raw SQ instruction counts
# (8 SQ counters + GRBM_GUI_ACTIVE).  Each pass profiles a plain bench run (warm-up and timed steps
# only).  Then tools/pmc_summary.py -> $OUT/<tag>_pmc_summary.json ($OUT defaults to bench_out/ in
# the repository).
# CONFIG=c5: the same passes over the C5 bench (bench.py --config c5).
TAG=${1:-pmc}
CFG=${CONFIG:-c3}
ROOT=${ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${OUT:-$ROOT/bench_out}
cd /tmp && export TMPDIR=/tmp && mkdir -p "$OUT"
run() {  # name, counters...
  local name=$1; shift
  timeout -s KILL 150 rocprofv3 --pmc "$@" --output-format csv -d "$OUT/${TAG}_$name" -o run \
    -- python3 "$ROOT/bench.py" --config "$CFG" --inflight 1 --steps 4 --warmup 1 \
    > "$OUT/${TAG}_$name.log" 2>&1
}
run FETCH FETCH_SIZE || exit $?
run WRITE WRITE_SIZE || exit $?
run COMPUTE MfmaUtil VALUBusy VALUUtilization SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_BUSY_CYCLES SQ_WAVES || exit $?
python3 "$ROOT/tools/pmc_summary.py" "$OUT/${TAG}_FETCH" "$OUT/${TAG}_WRITE" \
  "$OUT/${TAG}_COMPUTE" > "$OUT/${TAG}_pmc_summary.json"
