"""CPU-side checks of the boundary of world rays (include/sdm.h: sdm_query_world_segments / sdm_query_world_views /
sdm_debug_world_view_batch): the symbols are declared, exported and bound with their signatures, sdm_world_segment_hit has
the size, fields and offsets the header gives it, the new flag bit clashes with none of the query flags it is combined
with, the constants agree with the header, and every call is refused without a map."""
import ctypes as C
import inspect

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_query_world_segments", "sdm_query_world_views", "sdm_debug_world_view_batch")


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [5, 9, 2])))
    assert L.sdm_query_world_segments.argtypes[2] == C.c_int64 and L.sdm_query_world_segments.argtypes[4] == C.c_uint32
    assert L.sdm_query_world_views.argtypes[2] == C.c_int64 and L.sdm_query_world_views.argtypes[4:6] == [C.c_int32, C.c_int32]
    assert L.sdm_query_world_views.argtypes[8] == C.c_uint32 and L.sdm_debug_world_view_batch.argtypes[1] == C.c_int32
    want = dict(query_world_segments=["a", "b", "unknown_blocks", "ignore_movable", "on_device", "n", "out"],
                query_world_views=["views", "dirs", "reach_cells", "with_rays", "ignore_movable", "on_device", "n_views", "n_rays", "out", "rays_out"],
                set_world_view_batch=["max_views_in_flight"])
    for f, args in want.items():
        assert list(inspect.signature(getattr(binding.SdmMap, f)).parameters)[1:] == args, f
    sig = inspect.signature(binding.SdmMap.query_world_views).parameters
    assert sig["reach_cells"].default is inspect.Parameter.empty and sig["with_rays"].default is False and sig["ignore_movable"].default is False


def test_struct_size_fields_and_offsets():
    dt = binding.WORLD_SEGMENT_HIT
    assert_layout(dt, "sdm_world_segment_hit", 32)
    assert {f: dt.fields[f][1] for f in dt.names} == dict(t=0, cells=4, cell=8, track=20, label=22, occ=23, unknown=24, stamp=28)
    assert dt.fields["t"][0] == np.dtype("<f4") and dt.fields["cell"][0].base == np.dtype("<i4") and dt.fields["cell"][0].shape == (3,)
    assert dt.fields["occ"][0] == np.dtype("i1") and dt.fields["unknown"][0] == np.dtype("<i4") and dt.fields["stamp"][0] == np.dtype("<u4")
    # the views reuse sdm_view and sdm_view_gain as they are
    assert binding.VIEW.itemsize == 32 and binding.VIEW_GAIN.itemsize == 40


def test_flag_bits_and_constants():
    ignore = define("SDM_WORLD_RAYS_IGNORE_MOVABLE")
    assert ignore == binding.WORLD_RAYS_IGNORE_MOVABLE == 0x10
    others = [define("SDM_QUERY_ON_DEVICE"), define("SDM_QUERY_UNKNOWN_BLOCKS")]
    assert others == [binding.QUERY_ON_DEVICE, binding.QUERY_UNKNOWN_BLOCKS] == [1, 2]
    assert all(ignore & o == 0 for o in others) and bin(ignore).count("1") == 1
    assert define("SDM_WORLD_SEGMENT_MAX_CELLS") == binding.WORLD_SEGMENT_MAX_CELLS == 8192
    assert define("SDM_WORLD_VIEW_MAX_REACH") == binding.WORLD_VIEW_MAX_REACH == 255
    # the mask of the largest window: 511^3 bits, at least three of them in a pool of 64 MiB, its bit index within 32 bits
    S = 2 * binding.WORLD_VIEW_MAX_REACH + 1
    assert (64 << 20) // (-(-S ** 3 // 32) * 4) == 4 and S ** 3 < 1 << 32
    # a ray in a window visits at most 3 reach + 1 cells, fewer than a segment may
    assert 3 * binding.WORLD_VIEW_MAX_REACH + 1 < binding.WORLD_SEGMENT_MAX_CELLS


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ab, out = np.zeros((2, 6), np.float32), np.zeros(2, binding.WORLD_SEGMENT_HIT)
    views, dirs, gain = np.zeros(1, binding.VIEW), np.zeros((2, 3), np.float32), np.zeros(1, binding.VIEW_GAIN)
    assert L.sdm_query_world_segments(None, vp(ab), 2, vp(out), 0) == INV
    assert L.sdm_query_world_views(None, vp(views), 1, vp(dirs), 2, 4, vp(gain), vp(out), 0) == INV
    assert L.sdm_debug_world_view_batch(None, 1) == INV
