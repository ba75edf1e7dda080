"""CPU-side checks of the boundary of world ground reach (include/sdm.h: sdm_world_ground_reach_update /
sdm_get_world_ground_reach / sdm_query_world_ground_reach / sdm_world_ground_reach_paths): the symbols are declared,
exported and bound with their signatures, the three structs have the sizes, fields and offsets the header gives them, the
flag bits are distinct and agree with the header, the header's bytes per tile are the stated sum, and every call is
refused without a map."""
import ctypes as C
import inspect

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_ground_reach_update", "sdm_get_world_ground_reach", "sdm_query_world_ground_reach", "sdm_world_ground_reach_paths",
         "sdm_debug_world_ground_reach_tiles")
SIZES = dict(sdm_world_ground_reach_options=48, sdm_world_ground_reach_info=80, sdm_world_ground_reach_result=24)


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [5, 7, 6, 8, 2])))
    assert L.sdm_world_ground_reach_update.argtypes[4] == C.c_int64
    assert L.sdm_get_world_ground_reach.argtypes[3:6] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert L.sdm_query_world_ground_reach.argtypes[3] == C.c_int64 and L.sdm_query_world_ground_reach.argtypes[5] == C.c_uint32
    assert L.sdm_world_ground_reach_paths.argtypes[3:5] == [C.c_int64, C.c_int32] and L.sdm_world_ground_reach_paths.argtypes[7] == C.c_uint32
    # the same shapes as the world reach calls beside them
    for a, b in (("sdm_world_ground_reach_update", "sdm_world_reach_update"), ("sdm_get_world_ground_reach", "sdm_get_world_reach"),
                 ("sdm_query_world_ground_reach", "sdm_query_world_reach"), ("sdm_world_ground_reach_paths", "sdm_world_reach_paths")):
        assert getattr(L, a).argtypes == getattr(L, b).argtypes, a
    want = dict(world_ground_reach_update=["starts", "start_cells", "min_d2", "soft_d2", "penalty", "max_climb", "max_cost", "face_connected", "box"],
                world_ground_reach=["with_cost", "first", "cap"], query_world_ground_reach=["xyz", "cells", "on_device", "n", "out"],
                world_ground_reach_paths=["xyz", "cells", "max_len", "on_device", "n", "cells_out", "len_out", "fill"])
    for f, args in want.items():
        assert list(inspect.signature(getattr(binding.SdmMap, f)).parameters)[1:] == args, f
    sig = inspect.signature(binding.SdmMap.world_ground_reach_update).parameters
    assert [sig[k].default for k in want["world_ground_reach_update"]] == [None, None, 0, 0, 0, 0, 0, False, None]


def test_struct_sizes_fields_and_offsets():
    dtypes = dict(sdm_world_ground_reach_options=binding.WORLD_GROUND_REACH_OPTIONS, sdm_world_ground_reach_info=binding.WORLD_GROUND_REACH_INFO,
                  sdm_world_ground_reach_result=binding.WORLD_GROUND_REACH_RESULT)
    for name, dt in dtypes.items():
        assert_layout(dt, name, SIZES[name])
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_GROUND_REACH_OPTIONS) == dict(flags=0, min_d2=4, soft_d2=8, penalty=12, max_climb=16, max_cost=20, tmin=24, tmax=32,
                                                              pad=40)
    assert offsets(binding.WORLD_GROUND_REACH_INFO) == dict(n_tiles=0, n_starts_used=4, n_traversable=8, n_reached=12, max_cost_reached=16,
                                                           rounds=20, stamp=24, pad=28, options=32)
    assert offsets(binding.WORLD_GROUND_REACH_RESULT) == dict(cost=0, metres=4, col=8, level=16, next=18, status=19, pad=20)
    r = binding.WORLD_GROUND_REACH_RESULT
    assert r.fields["col"][0].base == np.dtype("<i4") and r.fields["col"][0].shape == (2,) and r.fields["level"][0] == np.dtype("<u2")
    assert r.fields["next"][0] == np.dtype("u1") and r.fields["status"][0] == np.dtype("u1") and r.fields["metres"][0] == np.dtype("<f4")
    assert binding.WORLD_GROUND_REACH_INFO.fields["options"][0] == binding.WORLD_GROUND_REACH_OPTIONS
    o = binding.WORLD_GROUND_REACH_OPTIONS
    assert o.fields["tmin"][0].base == np.dtype("<i4") and o.fields["pad"][0].shape == (2,)


def test_flag_bits_and_the_stated_bytes():
    bits = [define("SDM_WORLD_GROUND_REACH_" + n) for n in ("FACE_CONNECTED", "BOX")]
    assert bits == [binding.WORLD_GROUND_REACH_FACE_CONNECTED, binding.WORLD_GROUND_REACH_BOX] == [1, 2]
    # per tile: 64 costs, the traversable and the penalty word, 64 levels, eight neighbour ranks, the key, two slots of a 64-bit
    # key and a 32-bit rank, the list word
    per_tile = 64 * 4 + 8 + 8 + 64 * 2 + 8 * 4 + 4 + 2 * (8 + 4) + 4
    assert define("SDM_WORLD_GROUND_REACH_BYTES_PER_TILE") == binding.WORLD_GROUND_REACH_BYTES_PER_TILE == per_tile == 464
    # what a cost and a threshold have to hold: the largest penalised move below 2^17; R^2 + 1 of the largest radius
    assert 14 + 65535 < 1 << 17 and binding.WORLD_GROUND_MAX_RADIUS ** 2 + 1 < binding.WORLD_GROUND_NONE


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_GROUND_REACH_OPTIONS), np.zeros(1, binding.WORLD_GROUND_REACH_INFO)
    out = np.zeros(2, binding.WORLD_GROUND_REACH_RESULT)
    cells, rows, lens = np.zeros((2, 3), np.int32), np.zeros((2, 4, 3), np.int32), np.zeros(2, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n64 = C.c_int64(-7)
    assert L.sdm_world_ground_reach_update(None, vp(o), None, vp(cells), 2) == INV
    assert L.sdm_get_world_ground_reach(None, None, None, 0, 0, C.byref(n64), vp(info)) == INV and n64.value == -7
    assert L.sdm_query_world_ground_reach(None, None, vp(cells), 2, vp(out), 0) == INV
    assert L.sdm_world_ground_reach_paths(None, None, vp(cells), 2, 4, vp(rows), vp(lens), 0) == INV
    assert L.sdm_debug_world_ground_reach_tiles(None, C.byref(n64)) == INV and n64.value == -7
