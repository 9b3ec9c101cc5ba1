#!/bin/bash
# One GPU-box pass: build, GPU tests, bench, kernel-trace profile.
set -o pipefail
OUT=$(realpath -m "${OUT:-bench_out}")   # logs and profiles of this pass
mkdir -p $OUT
python -c "import __graft_entry__ as g; g.build()" > $OUT/build.log 2>&1 || exit 1
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1 || { tail -30 $OUT/pytest_gpu.log; exit 1; }
tail -3 $OUT/pytest_gpu.log
timeout -k 10 400 python bench.py --full ${BENCH_ARGS} > $OUT/bench.log 2>&1 || { tail -30 $OUT/bench.log; exit 1; }
tail -2 $OUT/bench.log
if [ -n "$PROFILE" ]; then
  R=$PWD
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run -- python3 $R/bench.py --full --steps 5 --warmup 2 > $OUT/prof.log 2>&1 || { tail -30 $OUT/prof.log; exit 1; }
  cd $R
fi
echo DONE
