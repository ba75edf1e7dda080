"""The kernels the builds over the world archive share (world_snapshot.hip) are exactly the box flag, the index, the 27
neighbour ranks (world reach's and world objects') and the active list, use no scratch and no LDS and spill no
vector and no scalar register.  Reads the code object's metadata only.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

WORLD_SNAPSHOT_KERNELS = ("k_ws_flag", "k_ws_index", "k_ws_neighbours", "k_ws_list")


def test_the_unit_is_listed():
    assert "world_snapshot" in hip_units()


def test_world_snapshot_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_snapshot")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_SNAPSHOT_KERNELS), list(meta)   # exactly the expected kernel set
    for k in WORLD_SNAPSHOT_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128 and lds[name] == 0, (k, v["vgpr_count"], lds[name])
