#!/bin/bash
# usage (GPU box): tools/prof_bench_csv.sh <tag> -> $out/<tag>_kernel_stats.csv : rocprofv3's own --stats table
set -u
tag=$1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export SDM_PROFILE_OUT=${SDM_PROFILE_OUT:-profile_out}; out=$SDM_PROFILE_OUT  # where the outputs go
mkdir -p $out
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/profcsv_$tag -o $tag -- python bench.py --full --no-cpu --no-dense --no-strong --steps 20 --warmup 5 > $out/${tag}_profcsv_bench.log 2>&1
find $out/profcsv_$tag -name "*kernel_stats.csv" -exec cp {} $out/${tag}_kernel_stats.csv \;
rm -rf $out/profcsv_$tag
