"""The kernels of world reach (world_reach.hip) use no scratch and spill no vector register, and none but the
26-connected path kernel - a descent loop round 27 loads under lane masks - spills a scalar one (into vector lanes, no
scratch; the ceiling is what a build with csrc/Makefile's flags gives).  Reads the code object's metadata only.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills

WORLD_REACH_KERNELS = ("k_wr_classify", "k_wr_inflateILi1", "k_wr_inflateILi2", "k_wr_seed",
                       "k_wr_relaxILb0", "k_wr_relaxILb1", "k_wr_reduce", "k_query_world_reachILb0", "k_query_world_reachILb1",
                       "k_world_reach_pathsILb0", "k_world_reach_pathsILb1")
SGPR_SPILL_CEILING = {"k_world_reach_pathsILb0": 6}   # every other kernel: 0


def test_the_unit_is_listed():
    assert "world_reach" in hip_units()


def test_world_reach_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_reach")
    meta, spills = kernels_meta(elf), sgpr_spills(elf)
    assert len(meta) == len(WORLD_REACH_KERNELS), list(meta)   # (no kernel of the frame, none of world_snapshot.hip)
    for k in WORLD_REACH_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0, (k, v)
        assert spills[name] <= SGPR_SPILL_CEILING.get(k, 0), (k, spills[name])
        assert int(v["vgpr_count"]) <= 128, (k, v["vgpr_count"])   # (two waves a SIMD for the 256-thread relaxation and more)
