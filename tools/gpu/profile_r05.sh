OUT=${1:?usage: bash tools/gpu/profile_r05.sh OUTDIR}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) || exit 1
cd "$(dirname "$0")/../.." || exit 1
bash tools/profile.sh r05 > $OUT/r05_profile.log 2>&1
(timeout 1200 python bench.py --full --steps 20 --warmup 5 > $OUT/r05_bench_full.json 2> $OUT/r05_bench_full.err; echo "exit $?" >> $OUT/r05_bench_full.err)
(timeout 600 python tools/time_p2.py 2>&1 | grep -v amdgpu > $OUT/r05_time_p2.txt)
(timeout 600 python tools/time_p2.py --form 3 2>&1 | grep -v amdgpu > $OUT/r05_time_p2_lockstep.txt)
tail -n 5 $OUT/r05_profile.log; tail -n 2 $OUT/r05_bench_full.err; cut -c1-300 $OUT/r05_bench_full.json
