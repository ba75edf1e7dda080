"""The kernels of the batched map queries (queries.hip) use no scratch.  (tests/test_isa_hygiene.py scans the object for
FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, kernels_meta

QUERY_KERNELS = ("k_query_points", "k_query_segments", "k_query_boxes")


def test_query_kernels_use_no_scratch(tmp_path):
    meta = kernels_meta(device_elf(tmp_path, "queries"))
    for k in QUERY_KERNELS:
        found = [v for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        assert int(found[0]["private_segment_fixed_size"]) == 0 and int(found[0]["vgpr_spill_count"]) == 0, (k, found)
