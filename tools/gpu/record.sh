#!/bin/bash
# ROOT: the repository; OUT: where the logs and records go (relative to ROOT), default bench_out
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${OUT:-bench_out}
# Final record of the tree: smoke(), default bench line, rocprof kernel stats, the counter passes (pmc_record.sh),
# cfg5 bench (with its CPU baseline) + kernel stats.  Usage: record.sh TAG
TAG=${1:-rec}
cd $ROOT && mkdir -p $OUT && export TMPDIR=/tmp
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$TAG.log 2>&1 || exit 1
tail -1 $OUT/smoke_$TAG.log
timeout -k 10 300 python -u bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit 1
head -c 400 $OUT/bench_$TAG.json; echo
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python3 -u bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --cfg5-steps 0 > $OUT/benchprof_$TAG.json 2> $OUT/benchprof_$TAG.err || exit 1
bash tools/gpu/pmc_record.sh $TAG > $OUT/pmc_$TAG.txt 2>&1 || exit 1
timeout -k 10 300 python -u bench.py --full --config 5 --steps 20 --warmup 5 --em-scale 0 > $OUT/bench_cfg5_$TAG.json 2> $OUT/bench_cfg5_$TAG.err || exit 1
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_cfg5_$TAG -o run -- python3 -u bench.py --full --config 5 --steps 5 --warmup 2 --no-cpu-baseline --em-scale 0 > /dev/null 2>&1 || exit 1
python - <<PY
import json
for f in ("$OUT/bench_$TAG.json", "$OUT/bench_cfg5_$TAG.json"):
    d = json.load(open(f)); print(f, d["value"], d["ms_per_step"], d["breakdown_ms"]["gamma"], d["breakdown_ms"]["em_hist"])
PY
echo done
