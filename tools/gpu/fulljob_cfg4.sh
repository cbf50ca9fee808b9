#!/bin/bash
# ROOT: the repository; OUT: where the logs and records go (relative to ROOT), default bench_out
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${OUT:-bench_out}
# Bench line + full-job rows.  Usage: bash tools/gpu/fulljob_cfg4.sh TAG RECORDS SHARD
TAG=${1:-job}; REC=${2:-1000000}; SHARD=${3:-0/1}
cd $ROOT
mkdir -p $OUT
export TMPDIR=/tmp
if [ "$4" != "nobench" ]; then
timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 3 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit 1
python - <<PY
import json; d=json.load(open("$OUT/bench_$TAG.json"))
print("value", d["value"], "ms/step", d["ms_per_step"]); print("breakdown", d["breakdown_ms"]); print("headline", d["hbm_headline_contract"]); print("roofline", d["roofline"]["frac"], d["roofline"]["algorithmic_bytes_per_launch"])
PY
fi
timeout -k 10 900 python -u tools/full_job.py --records $REC --shard $SHARD --out $OUT/fulljob_$TAG.json > $OUT/fulljob_$TAG.log 2>&1
rc=$?
tail -5 $OUT/fulljob_$TAG.log
exit $rc
