set -e
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
bash tools/chain_scaling.sh > $OUT/chain_scaling.txt 2>&1
cat $OUT/chain_scaling.txt
timeout -k 10 300 python bench.py --full --workload chimera512 --steps 3 --warmup 1 --no-search --cpu-rows 0 > $OUT/bench_chimera512.json 2> $OUT/bench_chimera512.err
timeout -k 10 400 python bench.py --full --workload rmf64 --steps 1 --warmup 0 --no-search --cpu-rows 0 > $OUT/bench_rmf64.json 2> $OUT/bench_rmf64.err
timeout -k 10 300 python bench.py --full --force-dist --steps 3 --warmup 1 --no-search --cpu-rows 0 > $OUT/bench_force_dist.json 2> $OUT/bench_force_dist.err
timeout -k 10 400 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
python - <<PY
import json
for f in ('bench_chimera512','bench_rmf64','bench_force_dist','bench_default'):
    d=json.loads([x for x in open('$OUT/%s.json' % f) if x.startswith('{')][-1]); print(f, d['value'])
PY
