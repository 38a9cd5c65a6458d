#!/bin/bash
# One gpurun call: GPU test suite, then (only if the suite was not killed / timed out) the bench line and the 2-rank rehearsal.
# usage: [OUT=dir] scripts/gpu_round.sh TAG [pytest args...]   (logs and JSON lines go to $OUT, default out/)
TAG=${1:-r03}; shift
OUT=${OUT:-out}
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -m gpu -q -s "$@" > "$OUT/${TAG}_tests.log" 2>&1
rc=$?
echo "pytest rc=$rc" >> "$OUT/${TAG}_tests.log"
tail -5 "$OUT/${TAG}_tests.log"
if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then exit $rc; fi
timeout -k 10 300 python bench.py --full --steps 5 --warmup 1 > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"
rb=$?
echo "bench rc=$rb"; cut -c1-600 "$OUT/${TAG}_bench.json"
if [ $rb -eq 124 ] || [ $rb -eq 137 ]; then exit $rb; fi
CEDARHIP_DIST_BACKEND=gloo timeout -k 10 300 python bench.py --full --gpus 2 --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/${TAG}_n2.json" 2> "$OUT/${TAG}_n2.err"
echo "n2 rc=$?"; tail -c 1500 "$OUT/${TAG}_n2.json"; tail -5 "$OUT/${TAG}_n2.err"
exit $rc
