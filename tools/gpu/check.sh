#!/bin/bash
# ROOT: the repository; OUT: where the logs and records go (relative to ROOT), default bench_out
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${OUT:-bench_out}
# One GPU round-trip: parity tests, bench, rocprof kernel stats.  Usage: bash tools/gpu/check.sh TAG
# Stops at the first step that times out, aborts or faults (only plain test failures continue).
TAG=${1:-run}
cd $ROOT
mkdir -p $OUT
timeout -k 10 650 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread > $OUT/tests_$TAG.log 2>&1
rc=$?
echo "pytest exit $rc" >> $OUT/tests_$TAG.log
tail -3 $OUT/tests_$TAG.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 180 python -u bench.py --full --steps 5 --warmup 2 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit 1
cat $OUT/bench_$TAG.json
export TMPDIR=/tmp
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python -u bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/benchprof_$TAG.json 2> $OUT/benchprof_$TAG.err
echo "prof exit $?" >> $OUT/benchprof_$TAG.err
