#!/bin/bash
# throughput of the 64 x 4K batch by number of sub-batch streams and hardware queues
#   scripts/exp_streams.sh OUT_DIR       (one bench line per setting: OUT_DIR/s<streams>_q<queues>.json)
O=$(mkdir -p "$1" && cd "$1" && pwd) || exit 1; cd "$(dirname "$0")/.."
for cfg in "8 2" "8 4" "12 8" "20 8" "20 16" "24 16"; do
  set -- $1 $cfg
  q=$2; n=$3
  GPU_MAX_HW_QUEUES=$q timeout 300 python bench.py --full --sub-batches $n --steps 3 --warmup 1 --no-cpu-baseline --no-phases > $O/s${n}_q$q.json 2> $O/err.log
  python - $O/s${n}_q$q.json $q $n <<'PY'
import json,sys
try:
    j=json.load(open(sys.argv[1])); print("queues", sys.argv[2], "streams asked", sys.argv[3], "used", j["config"]["streams_per_gpu"], "value", j["value"], "ms/step", j["ms_per_step"], "carve frac", j["roofline"]["frac"])
except Exception as e: print("failed", sys.argv[2:], e)
PY
done
