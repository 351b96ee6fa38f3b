#!/bin/bash
OUT=${1:?usage: bash tools/gpu/bench_quick.sh OUTDIR}
mkdir -p $OUT
timeout 900 python bench.py --full --steps 10 --warmup 3 --no-variants --no-config1 > $OUT/bench_quick.json 2> $OUT/bench_quick.err
echo "exit $?"
tail -3 $OUT/bench_quick.err
python - $OUT/bench_quick.json <<'P'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline'].get('traffic'))
print(json.dumps(d.get('behavior'), indent=1))
print(json.dumps(d.get('render',{}).get('bf16_shared_appearance')))
P
