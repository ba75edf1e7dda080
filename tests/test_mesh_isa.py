"""The kernels of the surface mesh (mesh.hip) use no scratch and spill no register, vector or scalar.  Reads the code
object's metadata only.  (tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of
the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills

MESH_KERNELS = ("k_mesh_classify", "k_mesh_faces", "k_mesh_corner_count", "k_mesh_emit", "k_mesh_vertices", "k_mesh_stats")


def test_the_unit_is_listed():
    assert "mesh" in hip_units()


def test_mesh_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "mesh")
    meta, spills = kernels_meta(elf), sgpr_spills(elf)
    assert len([n for n in meta if "k_mesh_" in n]) == len(MESH_KERNELS), list(meta)
    for k in MESH_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0, (k, v)
        assert spills[name] == 0, (k, spills[name])
