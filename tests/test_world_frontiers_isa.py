"""The kernels of the world frontiers (world_frontiers.hip) use no scratch, spill no vector and no scalar register, and
the brick-local labelling kernel holds its labels in registers: no LDS, as DESIGN.md 5n states.  Reads the code object's
metadata only.  (tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the
library.)"""
import os
import re
import subprocess

from tests.test_isa_hygiene import LLVM, device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills

WORLD_FRONTIERS_KERNELS = ("k_wf_index", "k_wf_classify", "k_wf_neighbours", "k_wf_mask", "k_wf_compact", "k_wf_label_localILb0",
                           "k_wf_label_localILb1", "k_wf_seamsILb0", "k_wf_seamsILb1", "k_wf_accumulate", "k_wf_flags", "k_wf_table")
LOCAL_LABEL_LDS_BYTES = 0              # eight labels a lane in registers, neighbours by lane shuffles


def lds_bytes(elf):
    """name -> group_segment_fixed_size from the code object's notes"""
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    blocks = re.split(r"\n\s+- \.agpr_count:|\n\s+- \.args:", out)
    found = {}
    for b in blocks:
        name, lds = re.search(r"\.name:\s+(\S+)", b), re.search(r"\.group_segment_fixed_size:\s+(\d+)", b)
        if name and lds and name.group(1).startswith("_Z"):
            found[name.group(1)] = int(lds.group(1))
    return found


def test_the_unit_is_listed():
    assert "world_frontiers" in hip_units()


def test_world_frontiers_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_frontiers")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_FRONTIERS_KERNELS), list(meta)   # (no kernel of the frame, none of frontiers.hip or world_snapshot.hip)
    for k in WORLD_FRONTIERS_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128, (k, v["vgpr_count"])
        if "k_wf_label_local" in k:
            assert lds[name] <= LOCAL_LABEL_LDS_BYTES, (k, lds[name])
