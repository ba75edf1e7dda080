"""The kernels of the world objects (world_objects.hip) are exactly those DESIGN.md 5v names, use no scratch, spill no vector
and no scalar register and stay within 128 VGPRs; the brick-local labelling kernel holds its keys, labels and neighbour
masks in registers - no LDS - and only the per-label counters use any, as 5v states.  Reads the code object's metadata
only.  (tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

WORLD_OBJECTS_KERNELS = ("k_wo_classify", "k_wo_compact", "k_wo_label_localILb0", "k_wo_label_localILb1", "k_wo_seamsILb0",
                         "k_wo_seamsILb1", "k_wo_roots", "k_wo_accumulate", "k_wo_flags", "k_wo_table", "k_wo_assign", "k_query_world_objects")
LDS_BYTES = {"k_wo_assign": 2048}      # 256 cell counts and 256 object counts a workgroup; every other kernel none


def test_the_unit_is_listed():
    assert "world_objects" in hip_units()


def test_world_objects_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_objects")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_OBJECTS_KERNELS), list(meta)   # (no kernel of the frame, none of another world unit)
    for k in WORLD_OBJECTS_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128, (k, v["vgpr_count"])
        assert lds[name] == LDS_BYTES.get(k, 0), (k, lds[name])
