#!/bin/bash
# usage (GPU box): tools/pmc_frame.sh <tag>  -> $out/<tag>_pmc.txt : per-kernel PMC averages of a few bench frames.
# Counter passes are separate runs (SQ: 8 slots, TCC: 4), never combined with sys/hip/hsa traces.
set -u
tag=$1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export SDM_PROFILE_OUT=${SDM_PROFILE_OUT:-profile_out}; out=$SDM_PROFILE_OUT  # where the outputs go
mkdir -p $out
run() {  # name, counters...
  name=$1; shift
  timeout 600 rocprofv3 --kernel-trace --output-format csv --pmc "$@" -d $out/pmc_${tag}_$name -o p -- \
    python bench.py --full --no-cpu --steps 3 --warmup 2 > $out/pmc_${tag}_$name.log 2>&1
}
run sq SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_VMEM
run tcc TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum GRBM_GUI_ACTIVE
run mem SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_SMEM SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VMEM TCP_PENDING_STALL_CYCLES_sum
python tools/pmc_summary.py $out/pmc_${tag}_sq $out/pmc_${tag}_tcc $out/pmc_${tag}_mem > $out/${tag}_pmc.txt 2>&1
