#!/bin/bash
# tools/quick_bench.sh <tag> <config> [name-filter] [ENV=..]: one bench.py run without the CPU baseline; prints ms_per_step
# and the eager per-kernel times whose name contains the filter
R=${GRAFT_REPO_ROOT:-.}
tag=$1; cfg=$2; filt=${3:-}; shift; shift; shift
OUT=${AB_OUT:-$R/ab_out}
mkdir -p $OUT
env "$@" timeout -k 10 240 python $R/bench.py --full --config $cfg --no-cpu-baseline > $OUT/$tag.json 2> $OUT/$tag.err || { tail -3 $OUT/$tag.err; exit 1; }
python3 - <<PY
import json
d = json.load(open("$OUT/$tag.json")); k = d.get("kernels") or d.get("kernels_eager_dispatch_clock") or {}
print("$tag", d["ms_per_step"], {n: (k[n]["avg_us"], k[n].get("launches")) for n in k if "$filt" and "$filt" in n})
PY
