"""The kernels of the instance table (instances.hip) use no scratch and spill no vector register.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta

INSTANCE_KERNELS = ("k_instances_accumulateILb1", "k_instances_accumulateILb0", "k_instances_finalize")


def test_the_unit_is_listed():
    assert "instances" in hip_units()


def test_instance_kernels_use_no_scratch(tmp_path):
    meta = kernels_meta(device_elf(tmp_path, "instances"))
    for k in INSTANCE_KERNELS:
        found = [v for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        assert int(found[0]["private_segment_fixed_size"]) == 0 and int(found[0]["vgpr_spill_count"]) == 0, (k, found)
