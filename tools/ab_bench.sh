#!/bin/bash
# quick A/B helper on a GPU box: tools/ab_bench.sh <tag> [env assignments] -> prints ms_per_step and the tail kernels' eager times
R=${GRAFT_REPO_ROOT:-.}
tag=$1; shift
OUT=${AB_OUT:-$R/ab_out}
mkdir -p $OUT
env "$@" timeout -k 10 240 python $R/bench.py --full --no-cpu-baseline --no-train-step --no-sweep --no-gather-leg > $OUT/$tag.json 2> $OUT/$tag.err || { tail -3 $OUT/$tag.err; exit 1; }
python3 - <<PY
import json
d = json.load(open("$OUT/$tag.json")); k = d["kernels_eager_dispatch_clock"]
print("$tag", d["ms_per_step"], d["ms_per_step_windows"]["median"], {n: k[n]["avg_us"] for n in k if "fwd_gemm" in n or "dgrad" in n or "multi" in n})
PY
