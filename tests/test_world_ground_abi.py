"""CPU-side checks of the boundary of the world ground layer (include/sdm.h: sdm_world_ground_update / sdm_get_world_ground /
sdm_query_world_ground / sdm_query_world_footprints): the symbols are declared, exported and bound with their signatures,
the four structs have the sizes, fields and offsets the header gives them, the flag bits are distinct and agree with the
header, the header's bytes per archived brick and per tile are the stated sums, the band helper, and every call is refused
without a map."""
import ctypes as C
import inspect

import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_ground_update", "sdm_get_world_ground", "sdm_query_world_ground", "sdm_query_world_footprints")
SIZES = dict(sdm_world_ground_options=80, sdm_world_ground_info=136, sdm_world_ground_result=40, sdm_world_footprint_result=40)


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [2, 8, 6, 5])))
    assert L.sdm_get_world_ground.argtypes[4:7] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert L.sdm_query_world_ground.argtypes[3] == C.c_int64 and L.sdm_query_world_ground.argtypes[5] == C.c_uint32
    assert L.sdm_query_world_footprints.argtypes[2] == C.c_int64 and L.sdm_query_world_footprints.argtypes[4] == C.c_uint32
    want = dict(world_ground_update=["up", "h_lo", "h_hi", "clearance", "max_step", "radius", "support_labels", "unknown_passable",
                                     "ignore_movable", "none_is_lethal", "absent_is_lethal", "box"],
                world_ground=["first", "cap"], query_world_ground=["xyz", "cells", "on_device", "n", "out"],
                query_world_footprints=["footprints", "on_device", "n", "out"])
    for f, args in want.items():
        assert list(inspect.signature(getattr(binding.SdmMap, f)).parameters)[1:] == args, f
    sig = inspect.signature(binding.SdmMap.world_ground_update).parameters
    assert [sig[k].default for k in want["world_ground_update"][6:]] == [None, False, False, False, False, None]


def test_struct_sizes_fields_and_offsets():
    dtypes = dict(sdm_world_ground_options=binding.WORLD_GROUND_OPTIONS, sdm_world_ground_info=binding.WORLD_GROUND_INFO,
                  sdm_world_ground_result=binding.WORLD_GROUND_RESULT, sdm_world_footprint_result=binding.WORLD_FOOTPRINT_RESULT)
    for name, dt in dtypes.items():
        assert_layout(dt, name, SIZES[name])
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_GROUND_OPTIONS) == dict(flags=0, up_axis=4, up_sign=8, h_lo=12, h_hi=16, clearance=20, max_step=24, radius=28,
                                                        tmin=32, tmax=40, support_labels=48)
    assert offsets(binding.WORLD_GROUND_INFO) == dict(n_tiles=0, level_min=4, level_max=8, stamp=12, n_ground=16, n_obstacle=24, n_none=32,
                                                     n_step=40, n_lethal=48, options=56)
    assert offsets(binding.WORLD_GROUND_RESULT) == dict(col=0, d2=8, surface=12, above=16, cell=20, dist=28, status=32, pad=36)
    assert offsets(binding.WORLD_FOOTPRINT_RESULT) == dict(n_cols=0, n_lethal=4, n_none=8, n_ground=12, n_absent=16, level_min=20, level_max=22,
                                                          min_d2=24, first_lethal=28, pad=36)
    r = binding.WORLD_GROUND_RESULT
    assert r.fields["col"][0].base == np.dtype("<i4") and r.fields["col"][0].shape == (2,) and r.fields["cell"][0] == binding.GROUND_CELL
    assert binding.WORLD_GROUND_INFO.fields["n_lethal"][0] == np.dtype("<i8") and binding.WORLD_GROUND_INFO.fields["options"][0] == binding.WORLD_GROUND_OPTIONS
    assert binding.WORLD_FOOTPRINT_RESULT.fields["first_lethal"][0].base == np.dtype("<i4")


def test_flag_bits_constants_and_the_stated_bytes():
    bits = [define("SDM_WORLD_GROUND_" + n) for n in ("UNKNOWN_PASSABLE", "IGNORE_MOVABLE", "NONE_IS_LETHAL", "ABSENT_IS_LETHAL", "BOX")]
    assert bits == [binding.WORLD_GROUND_UNKNOWN_PASSABLE, binding.WORLD_GROUND_IGNORE_MOVABLE, binding.WORLD_GROUND_NONE_IS_LETHAL,
                    binding.WORLD_GROUND_ABSENT_IS_LETHAL, binding.WORLD_GROUND_BOX] == [1, 2, 4, 8, 16]
    # the three cell flags are the block's
    assert bits[:3] == [binding.GROUND_UNKNOWN_PASSABLE, binding.GROUND_IGNORE_MOVABLE, binding.GROUND_NONE_IS_LETHAL]
    assert define("SDM_WORLD_GROUND_MAX_RADIUS") == binding.WORLD_GROUND_MAX_RADIUS == 16
    assert define("SDM_WORLD_GROUND_MAX_SPAN") == binding.WORLD_GROUND_MAX_SPAN == 4096
    assert define("SDM_WORLD_GROUND_NONE") == binding.WORLD_GROUND_NONE == 0xFFFF and define("SDM_WORLD_GROUND_FAR") == binding.WORLD_GROUND_FAR == 0xFFFFFFFE
    assert 16 * 16 < binding.WORLD_GROUND_NONE and 4095 + 255 < 0xFFFF       # what d2 and a relative height have to hold
    # per archived brick: the claim flag, the rank, two slots of a 64-bit key and a 32-bit rank
    assert define("SDM_WORLD_GROUND_BYTES_PER_ARCHIVED_BRICK") == 4 + 4 + 2 * (8 + 4)
    # per tile: 64 cells of 8 bytes, 64 distances of 2, the lethal word, the key, the sort's two keys and two values
    assert define("SDM_WORLD_GROUND_BYTES_PER_TILE") == 64 * 8 + 64 * 2 + 8 + 4 + 4 * 4


def test_the_band_helper():
    band = binding.world_ground_band
    assert band(0.25, (2, 1), -0.3, 1.0) == (-2, 4) and band(0.25, (1, -1), -0.3, 1.0) == (-5, 1)
    assert band(1.0, (0, 1), 0.0, 0.0) == (0, 0) and band(1.0, (0, -1), 0.0, 0.5) == (-1, -1)
    for bad in (((3, 1), 0, 1), ((0, 0), 0, 1), ((0, 1), 1, 0)):
        with pytest.raises(ValueError):
            band(0.25, *bad)


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_GROUND_OPTIONS), np.zeros(1, binding.WORLD_GROUND_INFO)
    o["up_axis"], o["up_sign"], o["radius"] = 2, 1, 4
    out, fout = np.zeros(2, binding.WORLD_GROUND_RESULT), np.zeros(2, binding.WORLD_FOOTPRINT_RESULT)
    cells, fps = np.zeros((2, 3), np.int32), np.zeros(2, binding.FOOTPRINT)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n64 = C.c_int64(-7)
    assert L.sdm_world_ground_update(None, vp(o)) == INV
    assert L.sdm_get_world_ground(None, None, None, None, 0, 0, C.byref(n64), vp(info)) == INV and n64.value == -7
    assert L.sdm_query_world_ground(None, None, vp(cells), 2, vp(out), 0) == INV
    assert L.sdm_query_world_footprints(None, vp(fps), 2, vp(fout), 0) == INV
