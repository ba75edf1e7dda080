"""The kernels of the frontiers (frontiers.hip) use no scratch and spill no vector register.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta

FRONTIER_KERNELS = ("k_frontier_classify", "k_frontier_mask", "k_frontier_compact", "k_frontier_labelILb1", "k_frontier_labelILb0",
                    "k_frontier_accumulate", "k_frontier_flags", "k_frontier_table")


def test_the_unit_is_listed():
    assert "frontiers" in hip_units()


def test_frontier_kernels_use_no_scratch(tmp_path):
    meta = kernels_meta(device_elf(tmp_path, "frontiers"))
    for k in FRONTIER_KERNELS:
        found = [v for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        assert int(found[0]["private_segment_fixed_size"]) == 0 and int(found[0]["vgpr_spill_count"]) == 0, (k, found)
