"""The kernels of world ground reach (world_ground_reach.hip) use no scratch, spill no vector and no scalar register, stay
within 128 VGPRs, and the relaxation's LDS is what DESIGN.md 5r states: none, its sweep reads the neighbours' costs across
the lanes.  Reads the code object's metadata only.  (tests/test_isa_hygiene.py scans the object for FLAT memory
instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

WORLD_GROUND_REACH_KERNELS = ("k_wgr_flag", "k_wgr_index", "k_wgr_neighbours", "k_wgr_classify", "k_wgr_seed", "k_wgr_relaxILb0",
                              "k_wgr_relaxILb1", "k_wgr_reduce", "k_query_world_ground_reachILb0", "k_query_world_ground_reachILb1",
                              "k_world_ground_reach_pathsILb0", "k_world_ground_reach_pathsILb1")
RELAX_LDS_BYTES = {"k_wgr_relaxILb0": 0, "k_wgr_relaxILb1": 0}


def test_the_unit_is_listed():
    assert "world_ground_reach" in hip_units()


def test_world_ground_reach_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_ground_reach")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_GROUND_REACH_KERNELS), list(meta)   # exactly the expected kernel set
    for k in WORLD_GROUND_REACH_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128, (k, v["vgpr_count"])
        assert lds[name] == RELAX_LDS_BYTES.get(k, 0), (k, lds[name])
