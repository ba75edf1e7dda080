export SDM_PROFILE_OUT=${SDM_PROFILE_OUT:-profile_out}; out=$SDM_PROFILE_OUT  # where the outputs go
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && mkdir -p $out
SDM_BENCH_SHARDED=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29561 timeout 600 rocprofv3 --kernel-trace --stats -d $out/prof_sh -o sh -- python bench.py --full --steps 20 --warmup 5 --no-cpu --no-stress --no-driven --no-adapter --no-dense --no-strong > $out/sh_prof.log 2>&1
python tools/trace_db.py $out/prof_sh/sh_results.db 4 > $out/r06_sharded_one_rank_kernel_stats.txt 2>&1
rm -rf $out/prof_sh
grep '"metric"' $out/sh_prof.log | tail -1 | python -c "
import sys, json
for l in sys.stdin:
    j = json.loads(l); print('sharded one rank: ms_per_step', j['ms_per_step'], j.get('collectives_us'))"
sed -n '/timeline/,$p' $out/r06_sharded_one_rank_kernel_stats.txt | head -60
