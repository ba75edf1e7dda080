#!/bin/bash
# usage (GPU box): tools/gpu_driven_sweep.sh [lib tags under build/ab ...]  ->  $out/driven_sweep.txt : the non-incremental sweep on a map grown by the
# `driven` scene, per launch and per kernel
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export SDM_PROFILE_OUT=${SDM_PROFILE_OUT:-profile_out}; out=$SDM_PROFILE_OUT  # where the outputs go
mkdir -p $out
export SDM_DRIVEN_CACHE=/tmp/sdm_driven_sweep_$$
{
  timeout 600 python tools/probes/driven_sweep.py
  for tag in "$@"; do SDM_LIB_PATH=build/ab/libsdm_$tag.so timeout 600 python tools/probes/driven_sweep.py; done
  rm -rf $out/dsw
  timeout 600 rocprofv3 --kernel-trace --output-format csv -d $out/dsw -o f -- python tools/probes/driven_sweep.py 2>&1 | grep driven_ms
  python - <<'PY'
import csv, glob, os
for f in glob.glob(os.environ["SDM_PROFILE_OUT"] + "/dsw/**/f_kernel_trace.csv", recursive=True):
    rows = [r for r in csv.DictReader(open(f)) if "occupancy_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for name in ("k_occupancy_scan", "k_occupancy_listed", "k_occupancy_dense"):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        print("  %-18s us per launch, grown map:" % name, " ".join("%.1f" % x for x in d[-8:]), "| empty map:", " ".join("%.1f" % x for x in d[2:5]))
PY
  rm -rf $out/dsw $SDM_DRIVEN_CACHE.*.npy
} > $out/driven_sweep.txt 2>&1
cat $out/driven_sweep.txt
