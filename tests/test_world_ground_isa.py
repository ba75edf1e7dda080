"""The kernels of the world ground layer (world_ground.hip) use no scratch, spill no vector and no scalar register, stay
within 128 VGPRs, and the distance kernel's LDS is what DESIGN.md 5q states.  Reads the code object's metadata only.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

WORLD_GROUND_KERNELS = ("k_wg_claim", "k_wg_keys", "k_wg_tiles", "k_wg_columnsILi0", "k_wg_columnsILi1", "k_wg_columnsILi2", "k_wg_cost",
                        "k_wg_distILi1", "k_wg_distILi2", "k_query_world_ground", "k_query_world_footprints")
# the lethal words of the (2 H + 1)^2 tiles, eight bytes per row of the halo
DIST_LDS_BYTES = {"k_wg_distILi1": 72 + 192, "k_wg_distILi2": 200 + 320}


def test_the_unit_is_listed():
    assert "world_ground" in hip_units()


def test_world_ground_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_ground")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_GROUND_KERNELS), list(meta)   # exactly the expected kernel set
    for k in WORLD_GROUND_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128, (k, v["vgpr_count"])
        if k in DIST_LDS_BYTES:
            assert lds[name] == DIST_LDS_BYTES[k], (k, lds[name])
        else:
            assert lds[name] == 0, (k, lds[name])
