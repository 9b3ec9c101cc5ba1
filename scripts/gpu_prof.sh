#!/bin/bash
# Kernel-trace profile of a short bench run: $OUT/prof/<tag>_kernel_stats.csv
set -o pipefail
OUT=$(realpath -m "${OUT:-bench_out}")   # logs and profiles of this pass
TAG=${TAG:-bench}
R=$PWD
mkdir -p $OUT/prof
python -c "import __graft_entry__ as g; g.build()" > $OUT/build.log 2>&1 || exit 1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o $TAG -- python3 $R/bench.py --full --steps ${STEPS:-5} --warmup 2 ${BENCH_ARGS} > $OUT/prof_$TAG.log 2>&1 || { tail -30 $OUT/prof_$TAG.log; exit 1; }
tail -1 $OUT/prof_$TAG.log
ls $OUT/prof
