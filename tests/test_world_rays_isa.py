"""The kernels of world rays (world_rays.hip) are exactly the two walks, use no scratch and no LDS, spill no vector and no
scalar register and stay within the vector registers DESIGN.md 5p reports, in blocks of 8.  Reads the code object's
metadata only.  (tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the
library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_layer_resources import allocated
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

# what the build reports: three waves per SIMD, 168 registers at most
VGPR_CEILING = {"k_world_segments": 157, "k_world_view_rays": 168}


def test_the_unit_is_listed():
    assert "world_rays" in hip_units()


def test_world_rays_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_rays")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(VGPR_CEILING), list(meta)   # (no kernel of the frame, none of another layer)
    for k in VGPR_CEILING:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert lds[name] == 0, (k, lds[name])
        if k in VGPR_CEILING:
            assert allocated(int(v["vgpr_count"])) <= allocated(VGPR_CEILING[k]) <= 168, (k, v["vgpr_count"])
