#!/bin/bash
# usage (GPU box): tools/round_profile.sh <tag>  ->  every tracked profile of a round from ONE tree state, under $out/
# (copy them to profiles/ afterwards; profiles/<tag>_sweep_pmc* are written in place):
#   <tag>_bench_c3.json              the line `python bench.py --full` prints
#   <tag>_kernel_stats.txt           rocprofv3 --kernel-trace --stats of the benchmark frames, launch by launch
#   <tag>_stress_kernel_stats.txt    the same on the busy scene
#   <tag>_sweep_pmc.json (+ CSVs)    HBM traffic of the sweep launches (FETCH_SIZE / WRITE_SIZE, separate passes)
#   <tag>_dense_pmc.txt              SQ counters of the sweep kernels on the dense case
#   <tag>_a7_sq.json                 SQ counters of the weight-update / visibility / birth / sweep kernels, C3 + busy scene
#   <tag>_driven.json, <tag>_driven_kernel_stats.txt   the `driven` leg alone and its kernel trace
#   <tag>_dense_split.txt            per-kernel times of the non-incremental sweep on the dense case + the streaming probes of this box
#   <tag>_clear.txt                  sdm_clear, ten calls
#   <tag>_driven_sweep.txt           the non-incremental sweep on a map the filter grew (150 frames of the driven scene), per launch and per kernel
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
tag=${1:-r03}
export SDM_PROFILE_OUT=${SDM_PROFILE_OUT:-profile_out}; out=$SDM_PROFILE_OUT  # where the outputs go
mkdir -p $out
timeout 900 python bench.py --full > $out/${tag}_bench_c3.json 2> $out/${tag}_bench_c3.err
tail -c 400 $out/${tag}_bench_c3.json; echo
SDM_GRAPH=0 tools/prof_bench.sh $tag
SDM_GRAPH=0 timeout 600 rocprofv3 --kernel-trace --stats -d $out/prof_${tag}_stress -o ${tag}_stress -- python bench.py --only-stress > $out/${tag}_stress_prof.log 2>&1
python tools/trace_db.py $out/prof_${tag}_stress/${tag}_stress_results.db 3 > $out/${tag}_stress_kernel_stats.txt 2>&1
rm -rf $out/prof_${tag}_stress
tools/pmc_sweep.sh $tag
tools/pmc_dense.sh $tag
tools/pmc_a7.sh $tag
tools/gpu_driven_stats.sh $tag > /dev/null 2>&1     # <tag>_driven.json, <tag>_driven_kernel_stats.txt
tools/gpu_dense_split.sh > /dev/null 2>&1; cp $out/dense_split.txt $out/${tag}_dense_split.txt
timeout 300 python tools/probes/clear_time.py 10 > $out/${tag}_clear.txt 2>&1
tools/gpu_driven_sweep.sh > /dev/null 2>&1; cp $out/driven_sweep.txt $out/${tag}_driven_sweep.txt
ls -la $out | grep $tag
