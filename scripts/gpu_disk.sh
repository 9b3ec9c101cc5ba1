#!/bin/bash
# Round-2 pass: GPU tests (strict), disk-mode bench small then full, synthetic harness.
set -o pipefail
OUT=$(realpath -m "${OUT:-bench_out}")   # logs and profiles of this pass
mkdir -p $OUT
df -h /tmp "${TMPDIR:-/tmp}" > $OUT/df.txt 2>&1; free -g >> $OUT/df.txt; nproc >> $OUT/df.txt
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
  > $OUT/pytest_gpu_all.log 2>&1 || { tail -40 $OUT/pytest_gpu_all.log; exit 1; }
tail -1 $OUT/pytest_gpu_all.log
timeout -k 10 300 python -u bench.py --full --mode disk --cols 125000000 --steps 10 --warmup 2 --topn-batches 0 \
  > $OUT/bench_disk_small.log 2>&1 || { tail -30 $OUT/bench_disk_small.log; exit 1; }
tail -1 $OUT/bench_disk_small.log
timeout -k 10 900 python -u bench.py --full ${BENCH_ARGS} > $OUT/bench_disk_full.log 2>&1 || { tail -30 $OUT/bench_disk_full.log; exit 1; }
tail -1 $OUT/bench_disk_full.log
