#!/bin/bash
# usage: tools/prof_bench.sh <tag>   (on the GPU box) -> $out/<tag>_kernel_stats.txt, <tag>_bench.json
set -u
tag=$1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export SDM_PROFILE_OUT=${SDM_PROFILE_OUT:-profile_out}; out=$SDM_PROFILE_OUT  # where the outputs go
mkdir -p $out
timeout 600 rocprofv3 --kernel-trace --stats -d $out/prof_$tag -o $tag -- python bench.py --full --no-cpu --no-dense --no-strong --steps 20 --warmup 5 > $out/${tag}_prof_bench.log 2>&1
python tools/trace_db.py $out/prof_$tag/${tag}_results.db 8 > $out/${tag}_kernel_stats.txt 2>&1
rm -rf $out/prof_$tag
