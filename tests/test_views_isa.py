"""The kernels of view scoring (views.hip) use no scratch and spill nothing, and mark cells with returned atomics.
(tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the library.)"""
from tests.test_isa_hygiene import device_elf, kernels_meta

VIEW_KERNELS = ("k_view_raysILi0E", "k_view_raysILi1E")   # marking and counting; clearing by a second walk


def test_view_kernels_use_no_scratch(tmp_path):
    meta = kernels_meta(device_elf(tmp_path, "views"))
    for k in VIEW_KERNELS:
        found = [v for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        assert int(found[0]["private_segment_fixed_size"]) == 0 and int(found[0]["vgpr_spill_count"]) == 0, (k, found)
        assert int(found[0]["vgpr_count"]) <= 128, (k, found)   # at least four waves per SIMD
