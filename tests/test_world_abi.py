"""CPU-side checks of the world archive's boundary (include/sdm.h: sdm_world_update / sdm_world_clear / sdm_get_world_info /
sdm_get_world_bricks / sdm_get_world_occupied / sdm_query_world_points / sdm_get_world_region): the symbols are declared,
exported and bound, the structs have the sizes and fields the header gives them, the constants agree with the header, and
every call is refused without a map."""
import ctypes as C

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_update", "sdm_world_clear", "sdm_get_world_info", "sdm_get_world_bricks", "sdm_get_world_occupied",
         "sdm_query_world_points", "sdm_get_world_region")


def test_symbols_are_declared_exported_and_bound():
    assert_bound(dict(zip(NAMES, [2, 1, 2, 6, 5, 5, 5])))
    for f in ("world_update", "world_info", "world_bricks", "world_occupied", "query_world", "world_region", "world_clear"):
        assert callable(getattr(binding.SdmMap, f)), f


def test_struct_sizes_and_fields():
    sizes = dict(sdm_world_options=16, sdm_world_brick=20, sdm_world_cell=8, sdm_world_info=80)
    dtypes = dict(sdm_world_options=binding.WORLD_OPTIONS, sdm_world_brick=binding.WORLD_BRICK, sdm_world_cell=binding.WORLD_CELL,
                  sdm_world_info=binding.WORLD_INFO)
    for name, size in sizes.items():
        assert_layout(dtypes[name], name, size)
    assert binding.WORLD_OPTIONS.fields["max_bricks"][1] == 8 and binding.WORLD_INFO.fields["dropped_total"][1] == 24


def test_constants_agree_with_the_header():
    assert define("SDM_WORLD_STATIC_ONLY") == binding.WORLD_STATIC_ONLY == 0x01
    assert define("SDM_WORLD_OBSERVED_ONLY") == binding.WORLD_OBSERVED_ONLY == 0x02
    # per brick of capacity: the words, the header, two hash slots (key and pool slot), four sort words and a count
    assert define("SDM_WORLD_BYTES_PER_BRICK") == 512 * 4 + binding.WORLD_BRICK.itemsize + 2 * (8 + 4) + 4 * 4 + 4
    assert binding.WORLD_UNKNOWN_WORD == 0xFF000000


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_OPTIONS), np.zeros(1, binding.WORLD_INFO)
    bricks, cells = np.zeros(2, binding.WORLD_BRICK), np.zeros((2, 512), np.uint32)
    pts, xyz, out = np.zeros(4, binding.POINT), np.zeros((4, 3), np.float32), np.zeros(4, binding.WORLD_CELL)
    lo, size, words = np.zeros(3, np.int32), np.ones(3, np.int32), np.zeros(1, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = C.c_int64(-7)
    assert L.sdm_world_update(None, None) == INV and L.sdm_world_update(None, vp(o)) == INV and L.sdm_world_clear(None) == INV
    assert L.sdm_get_world_info(None, None) == INV and L.sdm_get_world_info(None, vp(info)) == INV
    assert L.sdm_get_world_bricks(None, None, None, 0, 0, None) == INV and L.sdm_get_world_bricks(None, vp(bricks), vp(cells), 0, 2, C.byref(n)) == INV
    assert L.sdm_get_world_occupied(None, None, 0, None, 0) == INV and L.sdm_get_world_occupied(None, vp(pts), 4, C.byref(n), 0) == INV
    assert L.sdm_query_world_points(None, None, 0, None, 0) == INV and L.sdm_query_world_points(None, vp(xyz), 4, vp(out), 0) == INV
    assert L.sdm_get_world_region(None, None, None, None, 0) == INV and L.sdm_get_world_region(None, vp(lo), vp(size), vp(words), 0) == INV
    assert n.value == -7 and not info.view(np.uint8).any() and not out.view(np.uint8).any()   # nothing was written
