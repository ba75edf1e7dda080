"""The kernels of the travel-cost field (reach.hip) use no scratch and spill no register, vector or scalar.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
import os
import re
import subprocess

from tests.test_isa_hygiene import LLVM, device_elf, hip_units, kernels_meta

# the relaxation is one kernel per connectivity and tile extent (4 or 8 cells an axis)
RELAX_KERNELS = tuple("k_reach_relaxILb%dELi%dELi%dELi%dEE" % (f, x, y, z) for f in (0, 1) for x in (2, 3) for y in (2, 3) for z in (2, 3))
REACH_KERNELS = ("k_reach_classifyILb0", "k_reach_classifyILb1", "k_reach_seed", "k_reach_list", "k_reach_reduce", "k_query_reachILb0",
                 "k_query_reachILb1", "k_reach_pathsILb0", "k_reach_pathsILb1") + RELAX_KERNELS


def sgpr_spills(elf):
    """name -> sgpr_spill_count from the code object's notes (a kernel's block begins with its .agpr_count or .args and
    holds its .name before its .sgpr_spill_count)"""
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    spills, name = {}, None
    for line in out.splitlines():
        m = re.match(r"\s+\.(name|sgpr_spill_count):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "name":
            name = m.group(2)
        else:
            spills[name] = int(m.group(2))
    return spills


def test_the_unit_is_listed():
    assert "reach" in hip_units()


def test_reach_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "reach")
    meta, spills = kernels_meta(elf), sgpr_spills(elf)
    assert len([n for n in meta if "k_reach_" in n or "k_query_reach" in n]) == len(REACH_KERNELS), list(meta)
    for k in REACH_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0, (k, v)
        assert spills[name] == 0, (k, spills[name])
