"""CPU-side checks of the ground layer's boundary (include/sdm.h: sdm_ground_update / sdm_get_ground / sdm_query_ground /
sdm_query_footprints): the symbols are declared, exported and bound, the structs have the sizes and fields the header
gives them, the constants agree with the header, and the calls that need no device are refused as the header says."""
import ctypes as C

from semantic_dsp_map_amd import binding
from tests.abi_checks import HEADER, assert_bound, assert_layout, define

NAMES = ("sdm_ground_update", "sdm_get_ground", "sdm_query_ground", "sdm_query_footprints")


def test_symbols_are_declared_exported_and_bound():
    assert_bound(dict(zip(NAMES, [2, 5, 5, 5])))
    for f in ("ground_update", "ground", "query_ground", "query_footprints"):
        assert callable(getattr(binding.SdmMap, f)), f
    assert callable(binding.ground_band) and callable(binding.label_mask)


def test_struct_sizes_and_fields():
    sizes = dict(sdm_ground_options=60, sdm_ground_cell=8, sdm_ground_info=104, sdm_ground_result=32, sdm_footprint=24, sdm_footprint_result=32)
    dtypes = dict(sdm_ground_options=binding.GROUND_OPTIONS, sdm_ground_cell=binding.GROUND_CELL, sdm_ground_info=binding.GROUND_INFO,
                  sdm_ground_result=binding.GROUND_RESULT, sdm_footprint=binding.FOOTPRINT, sdm_footprint_result=binding.FOOTPRINT_RESULT)
    for name, size in sizes.items():
        assert_layout(dtypes[name], name, size)
    assert binding.GROUND_RESULT.fields["cell"][0] == binding.GROUND_CELL and binding.GROUND_INFO.fields["options"][0] == binding.GROUND_OPTIONS


def test_constants_agree_with_the_header():
    assert define("SDM_GROUND_UNKNOWN_PASSABLE") == binding.GROUND_UNKNOWN_PASSABLE == 1
    assert define("SDM_GROUND_IGNORE_MOVABLE") == binding.GROUND_IGNORE_MOVABLE == 2
    assert define("SDM_GROUND_NONE_IS_LETHAL") == binding.GROUND_NONE_IS_LETHAL == 4
    assert binding.GROUND_NO_LEVEL == 0xFFFF and binding.GROUND_MAX_FOOTPRINT_CELLS == 64
    assert "half_len + half_wid > 64 * voxel_size" in HEADER


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    import numpy as np
    o, pts, out = np.zeros(1, binding.GROUND_OPTIONS), np.zeros(3, np.float32), np.zeros(1, binding.GROUND_RESULT)
    fp, res = np.zeros(1, binding.FOOTPRINT), np.zeros(1, binding.FOOTPRINT_RESULT)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.sdm_ground_update(None, None) == INV and L.sdm_ground_update(None, vp(o)) == INV
    assert L.sdm_get_ground(None, None, None, None, None) == INV
    assert L.sdm_query_ground(None, None, 0, None, 0) == INV and L.sdm_query_ground(None, vp(pts), 1, vp(out), 0) == INV
    assert L.sdm_query_footprints(None, None, 0, None, 0) == INV and L.sdm_query_footprints(None, vp(fp), 1, vp(res), 0) == INV
