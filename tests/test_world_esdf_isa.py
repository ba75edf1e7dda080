"""The kernels of the world distance field (world_esdf.hip) use no scratch, spill no vector and no scalar register, stay
within 128 VGPRs, and the build kernel's LDS is what DESIGN.md 5o states.  Reads the code object's metadata only.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

WORLD_ESDF_KERNELS = ("k_we_classify", "k_we_buildILi1", "k_we_buildILi2", "k_query_world_distance")
# obstacle words, the x pass' bytes, the y pass' words, the neighbours' slots, the waves' two counts
BUILD_LDS_BYTES = {"k_we_buildILi1": 1728 + 4608 + 6144 + 112 + 32, "k_we_buildILi2": 8000 + 12800 + 10240 + 512 + 32}


def test_the_unit_is_listed():
    assert "world_esdf" in hip_units()


def test_world_esdf_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_esdf")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_ESDF_KERNELS), list(meta)   # (no kernel of the frame, none of esdf.hip or world_snapshot.hip)
    for k in WORLD_ESDF_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128, (k, v["vgpr_count"])
        if k in BUILD_LDS_BYTES:
            assert 0 < lds[name] <= BUILD_LDS_BYTES[k] < 64 * 1024, (k, lds[name])
        else:
            assert lds[name] == 0, (k, lds[name])
