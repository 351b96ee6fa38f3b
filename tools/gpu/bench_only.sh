#!/bin/bash
OUT=${1:?usage: bash tools/gpu/bench_only.sh OUTDIR}
mkdir -p $OUT
timeout 900 python bench.py --full --no-variants --no-config1 --no-render --no-cpu-baseline > $OUT/bench_short.json 2> /dev/null
python - $OUT/bench_short.json <<'P'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("SPREAD", round(d['value'],1), round(d['ms_per_step'],3), round(d['roofline']['frac'],4), round(d['roofline']['whole_step_frac'],4))
P
