"""CPU-side checks of the boundary of world reach (include/sdm.h: sdm_world_reach_update / sdm_get_world_reach /
sdm_query_world_reach / sdm_world_reach_paths): the symbols are declared, exported and bound with their signatures, the
three structs have the sizes, fields and offsets the header gives them, the flag bits are distinct and agree with the
header, and every call is refused without a map."""
import ctypes as C
import inspect

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_reach_update", "sdm_get_world_reach", "sdm_query_world_reach", "sdm_world_reach_paths")


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [5, 7, 6, 8])))
    assert L.sdm_world_reach_update.argtypes[4] is C.c_int64
    assert L.sdm_get_world_reach.argtypes[3:6] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert L.sdm_query_world_reach.argtypes[3] is C.c_int64 and L.sdm_query_world_reach.argtypes[5] is C.c_uint32
    assert L.sdm_world_reach_paths.argtypes[3:5] == [C.c_int64, C.c_int32] and L.sdm_world_reach_paths.argtypes[7] is C.c_uint32
    want = dict(world_reach_update=["starts", "start_cells", "inflate", "max_cost", "face_connected", "through_unknown", "ignore_movable", "box"],
                world_reach=["with_cost", "first", "cap"], query_world_reach=["xyz", "cells", "on_device", "n", "out"],
                world_reach_paths=list(inspect.signature(binding.SdmMap.reach_paths).parameters)[1:])
    for f, args in want.items():
        assert list(inspect.signature(getattr(binding.SdmMap, f)).parameters)[1:] == args, f


def test_struct_sizes_fields_and_offsets():
    dtypes = dict(sdm_world_reach_options=binding.WORLD_REACH_OPTIONS, sdm_world_reach_info=binding.WORLD_REACH_INFO,
                  sdm_world_reach_result=binding.WORLD_REACH_RESULT)
    sizes = dict(sdm_world_reach_options=40, sdm_world_reach_info=40, sdm_world_reach_result=24)
    for name, size in sizes.items():
        assert_layout(dtypes[name], name, size)
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_REACH_OPTIONS) == dict(flags=0, inflate=4, max_cost=8, pad=12, bmin=16, bmax=28)
    assert offsets(binding.WORLD_REACH_INFO) == dict(n_bricks=0, n_starts_used=4, n_traversable=8, n_reached=12, max_cost_reached=16, rounds=20,
                                                     flags=24, inflate=28, max_cost=32, stamp=36)
    assert offsets(binding.WORLD_REACH_RESULT) == dict(cost=0, metres=4, cell=8, next=20, status=21, pad=22)
    assert binding.WORLD_REACH_RESULT.fields["cell"][0].shape == (3,) and binding.WORLD_REACH_RESULT.fields["cell"][0].base == np.dtype("<i4")


def test_flag_bits_are_distinct_and_agree_with_the_header():
    bits = [define("SDM_WORLD_REACH_FACE_CONNECTED"), define("SDM_WORLD_REACH_THROUGH_UNKNOWN"), define("SDM_WORLD_REACH_IGNORE_MOVABLE"),
            define("SDM_WORLD_REACH_BOX")]
    assert bits == [binding.WORLD_REACH_FACE_CONNECTED, binding.WORLD_REACH_THROUGH_UNKNOWN, binding.WORLD_REACH_IGNORE_MOVABLE,
                    binding.WORLD_REACH_BOX] == [1, 2, 4, 8]
    assert all(b and not b & (b - 1) for b in bits) and len(set(bits)) == 4


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_REACH_OPTIONS), np.zeros(1, binding.WORLD_REACH_INFO)
    p, res, lens = np.zeros((2, 3), np.float32), np.zeros(2, binding.WORLD_REACH_RESULT), np.full(2, -7, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = C.c_int64(-7)
    assert L.sdm_world_reach_update(None, vp(o), vp(p), None, 2) == INV
    assert L.sdm_get_world_reach(None, None, None, 0, 0, C.byref(n), vp(info)) == INV and n.value == -7
    assert L.sdm_query_world_reach(None, vp(p), None, 2, vp(res), 0) == INV
    assert L.sdm_world_reach_paths(None, vp(p), None, 2, 0, None, vp(lens), 0) == INV and lens.tolist() == [-7, -7]
