#!/bin/bash
# Round-end style pass: all GPU tests, smoke, full bench, kernel-trace profile.
set -o pipefail
OUT=$(realpath -m "${OUT:-bench_out}")   # logs and profiles of this pass
mkdir -p $OUT/prof
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
  > $OUT/pytest_gpu_all.log 2>&1 || { tail -40 $OUT/pytest_gpu_all.log; exit 1; }
tail -1 $OUT/pytest_gpu_all.log
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" || exit 1
timeout -k 10 600 python -u bench.py --full > $OUT/bench_full.log 2>&1 || { tail -20 $OUT/bench_full.log; exit 1; }
tail -1 $OUT/bench_full.log
R=$PWD
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o final -- \
  python3 $R/bench.py --full --steps 5 --warmup 2 > $OUT/prof_final.log 2>&1 || { tail -20 $OUT/prof_final.log; exit 1; }
echo PROFILED
