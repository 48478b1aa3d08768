#!/bin/bash
# FPS lab counters (rounds, scans, rescans per reason, per-wave phase clocks) at the C3 sizes, then
# the C5 bench (N = 65536, K = 256, fp16 features) with its latency and rooflines (--full).  Build
# the lab first on the CPU: make -C tools/fps_lab fps_lab.  Logs go to $OUT (default: bench_out/ in
# the repository).  Usage: tools/gpu_fps_c5.sh <tag>
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/bench_out}
cd "$ROOT" && mkdir -p "$OUT"
tag=${1:-fc}
timeout -k 10 240 ./tools/fps_lab/fps_lab 16 16384 10000 > "$OUT/${tag}_fps_lab.log" 2>&1 || exit $?
timeout -k 10 120 ./tools/fps_lab/fps_lab 16 10000 10000 >> "$OUT/${tag}_fps_lab.log" 2>&1 || exit $?
# variant lab binaries, when any were built from an edited tree (hipcc ... -o fps_lab_<name>)
for v in tools/fps_lab/fps_lab_*; do
  [ -x "$v" ] || continue
  echo "== $v" >> "$OUT/${tag}_fps_lab.log"
  timeout -k 10 240 "$v" 16 16384 10000 >> "$OUT/${tag}_fps_lab.log" 2>&1 || exit $?
  timeout -k 10 120 "$v" 16 10000 10000 >> "$OUT/${tag}_fps_lab.log" 2>&1 || exit $?
done
timeout -k 10 600 python bench.py --full --config c5 --no-cpu-baseline > "$OUT/${tag}_bench_c5.log" 2>&1
