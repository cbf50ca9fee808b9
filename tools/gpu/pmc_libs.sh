#!/bin/bash
# ROOT: the repository; OUT: where the logs and records go (relative to ROOT), default bench_out
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${OUT:-bench_out}
# SQ / LDS / TA counter passes of a short bench run per library build (A = in-tree, then candidates),
# summarised per kernel matching REGEX (tools/pmc_summary.py).
# Usage: bash tools/gpu/pmc_libs.sh "ab_x.so ..." [REGEX]
cd $ROOT && mkdir -p $OUT && export TMPDIR=/tmp
LIBS=${1:-}; RX=${2:-k_filter}
B="python -u bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --em-scale 0"
for lib in A $LIBS; do
  if [ $lib == A ]; then unset SPLINK_AMD_LIB; else export SPLINK_AMD_LIB=$ROOT/splink_amd/$lib; fi
  pass() { local n=$1; shift; timeout -s KILL 200 rocprofv3 --pmc "$@" --kernel-trace --output-format csv -d $OUT/pmc${n}_$lib -o run -- $B > $OUT/pmc${n}_$lib.log 2>&1; }
  pass 1 SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_BRANCH SQ_ACTIVE_INST_VALU || exit 1
  pass 2 SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SMEM SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_VMEM_WR || exit 1
  pass 3 TA_TA_BUSY_sum TA_ADDR_STALLED_BY_TC_CYCLES_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_PENDING_STALL_CYCLES_sum GRBM_GUI_ACTIVE GRBM_COUNT || exit 1
  echo "== $lib"
  python tools/pmc_summary.py $OUT/pmc1_$lib $OUT/pmc2_$lib $OUT/pmc3_$lib --match "$RX" --json $OUT/pmc_$lib.json 2>&1 | head -30
done
