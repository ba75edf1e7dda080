"""CPU-side checks of the boundary of the world distance field (include/sdm.h: sdm_world_esdf_update / sdm_get_world_esdf /
sdm_query_world_distance): the symbols are declared, exported and bound with their signatures, the three structs have the
sizes, fields and offsets the header gives them, the flag bits are distinct and agree with the header, the header's bytes
per archived brick and per field brick are the stated sums, and every call is refused without a map."""
import ctypes as C
import inspect

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_esdf_update", "sdm_get_world_esdf", "sdm_query_world_distance")


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [2, 8, 6])))
    assert L.sdm_get_world_esdf.argtypes[4:7] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert L.sdm_query_world_distance.argtypes[3] == C.c_int64 and L.sdm_query_world_distance.argtypes[5] == C.c_uint32
    want = dict(world_esdf_update=["radius", "unknown_is_obstacle", "static_only", "box"], world_esdf=["first", "cap"],
                query_world_distance=["xyz", "cells", "on_device", "n", "out"])
    for f, args in want.items():
        assert list(inspect.signature(getattr(binding.SdmMap, f)).parameters)[1:] == args, f
    sig = inspect.signature(binding.SdmMap.world_esdf_update).parameters
    assert sig["radius"].default is inspect.Parameter.empty and [sig[k].default for k in want["world_esdf_update"][1:]] == [False, False, None]
    sig = inspect.signature(binding.SdmMap.query_world_distance).parameters
    assert [sig[k].default for k in want["query_world_distance"]] == [None, None, False, None, None]


def test_struct_sizes_fields_and_offsets():
    dtypes = dict(sdm_world_esdf_options=binding.WORLD_ESDF_OPTIONS, sdm_world_esdf_info=binding.WORLD_ESDF_INFO,
                  sdm_world_distance_result=binding.WORLD_DISTANCE_RESULT)
    for name, dt in dtypes.items():
        assert_layout(dt, name, 32)
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_ESDF_OPTIONS) == dict(flags=0, radius=4, bmin=8, bmax=20)
    assert offsets(binding.WORLD_ESDF_INFO) == dict(n_bricks=0, flags=4, radius=8, stamp=12, n_obstacle_cells=16, n_near_cells=24)
    assert offsets(binding.WORLD_DISTANCE_RESULT) == dict(cell=0, nearest=12, d2=24, distance=28)
    r = binding.WORLD_DISTANCE_RESULT
    assert r.fields["cell"][0].base == np.dtype("<i4") and r.fields["nearest"][0].shape == (3,) and r.fields["distance"][0] == np.dtype("<f4")
    assert binding.WORLD_ESDF_INFO.fields["n_near_cells"][0] == np.dtype("<i8") and binding.WORLD_ESDF_OPTIONS.fields["bmax"][0].shape == (3,)


def test_flag_bits_constants_and_the_stated_bytes():
    bits = [define("SDM_WORLD_ESDF_UNKNOWN_IS_OBSTACLE"), define("SDM_WORLD_ESDF_STATIC_ONLY"), define("SDM_WORLD_ESDF_BOX")]
    assert bits == [binding.WORLD_ESDF_UNKNOWN_IS_OBSTACLE, binding.WORLD_ESDF_STATIC_ONLY, binding.WORLD_ESDF_BOX] == [1, 2, 4]
    assert define("SDM_WORLD_ESDF_MAX_RADIUS") == binding.WORLD_ESDF_MAX_RADIUS == 16
    assert define("SDM_WORLD_ESDF_NONE") == binding.WORLD_ESDF_NONE == 0xFFFF and define("SDM_WORLD_ESDF_FAR") == binding.WORLD_ESDF_FAR == 0xFFFFFFFE
    # per archived brick: the box flag, the rank, eight 64-bit obstacle words
    assert define("SDM_WORLD_ESDF_BYTES_PER_ARCHIVED_BRICK") == 4 + 4 + 8 * 8
    # per brick of the field: 512 packed words (10 bits of d2, 3 x 6 bits of offset), the coordinates (two words), two hash
    # slots of a 64-bit key and a 32-bit rank
    assert define("SDM_WORLD_ESDF_BYTES_PER_BRICK") == 512 * 4 + 2 * 4 + 2 * (8 + 4)
    assert 16 * 16 < (1 << 10) - 1 and 2 * 16 + 1 <= 1 << 6     # what the packed word has to hold


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_ESDF_OPTIONS), np.zeros(1, binding.WORLD_ESDF_INFO)
    o["radius"] = 4
    out, cells = np.zeros(2, binding.WORLD_DISTANCE_RESULT), np.zeros((2, 3), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n64 = C.c_int64(-7)
    assert L.sdm_world_esdf_update(None, vp(o)) == INV
    assert L.sdm_get_world_esdf(None, None, None, None, 0, 0, C.byref(n64), vp(info)) == INV and n64.value == -7
    assert L.sdm_query_world_distance(None, None, vp(cells), 2, vp(out), 0) == INV
