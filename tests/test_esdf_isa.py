"""The kernels of the distance field (esdf.hip) use no scratch and spill nothing.  (tests/test_isa_hygiene.py scans the
object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, kernels_meta

ESDF_KERNELS = ("k_esdf_x", "k_esdf_envILi1", "k_esdf_envILi2", "k_query_distance")


def test_esdf_kernels_use_no_scratch(tmp_path):
    meta = kernels_meta(device_elf(tmp_path, "esdf"))
    for k in ESDF_KERNELS:
        found = [v for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        assert int(found[0]["private_segment_fixed_size"]) == 0 and int(found[0]["vgpr_spill_count"]) == 0, (k, found)
