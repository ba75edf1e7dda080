"""The kernels of the world archive (world.hip) use no scratch and spill no register, vector or scalar.  Reads the code
object's metadata only.  (tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of
the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills

WORLD_KERNELS = ("k_world_mark", "k_world_merge", "k_world_finish", "k_world_order_lo", "k_world_order_hi", "k_world_gather",
                 "k_world_occ_count", "k_world_occ_emit", "k_world_query", "k_world_region")


def test_the_unit_is_listed():
    assert "world" in hip_units()


def test_world_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world")
    meta, spills = kernels_meta(elf), sgpr_spills(elf)
    assert len([n for n in meta if "k_world_" in n]) == len(WORLD_KERNELS) == len(meta), list(meta)
    for k in WORLD_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0, (k, v)
        assert spills[name] == 0, (k, spills[name])
