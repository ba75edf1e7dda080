"""The kernels of the world mesh (world_mesh.hip) are exactly the ones DESIGN.md 5t names, use no scratch and no LDS, spill
no vector and no scalar register and stay within 128 VGPRs.  Reads the code object's metadata only.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

WORLD_MESH_KERNELS = ("k_wm_clear", "k_wm_classify", "k_wm_neighbours", "k_wm_faces", "k_wm_vflag", "k_wm_sums", "k_wm_vkeysE", "k_wm_vkeys_hi",
                      "k_wm_vrank", "k_wm_owners", "k_wm_emit", "k_wm_vertices")


def test_the_unit_is_listed():
    assert "world_mesh" in hip_units()


def test_world_mesh_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_mesh")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_MESH_KERNELS), list(meta)   # (no kernel of the frame, none of mesh.hip or world_snapshot.hip)
    for k in WORLD_MESH_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128 and lds[name] == 0, (k, v["vgpr_count"], lds[name])   # no kernel uses LDS
