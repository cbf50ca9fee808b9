#!/bin/bash
# ROOT: the repository; OUT: where the logs and records go (relative to ROOT), default bench_out
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${OUT:-bench_out}
# A/B of library builds on the cfg5 columns (bench.py --config 5), alternating; parity via the cfg5 tests.
# Usage: bash tools/gpu/ab_cfg5.sh "ab_x.so ab_y.so"
cd $ROOT && mkdir -p $OUT && export TMPDIR=/tmp
LIBS=${1:-}
for lib in $LIBS; do
  SPLINK_AMD_LIB=$ROOT/splink_amd/$lib timeout -k 10 300 python -u -m pytest tests -m gpu -q -x --timeout 200 --timeout-method thread -k "cfg5_address" > $OUT/tests_$lib.log 2>&1
  rc=$?; echo "$lib pytest exit $rc: $(tail -1 $OUT/tests_$lib.log)"
  if [ $rc -ne 0 ]; then exit $rc; fi
done
: > $OUT/abcfg5.log
for rep in 1 2; do
  for lib in A $LIBS; do
    if [ $lib == A ]; then unset SPLINK_AMD_LIB; else export SPLINK_AMD_LIB=$ROOT/splink_amd/$lib; fi
    timeout -k 10 240 python -u bench.py --full --config 5 --steps 10 --warmup 3 --no-cpu-baseline --em-scale 0 > $OUT/abcfg5_$lib.json 2>/dev/null || exit 1
    python -c "
import json; d=json.load(open('$OUT/abcfg5_$lib.json')); b=d['breakdown_ms']
print('$lib', 'ms/step %.4f' % d['ms_per_step'], 'gamma %.4f' % b['gamma'])" >> $OUT/abcfg5.log
  done
done
cat $OUT/abcfg5.log
