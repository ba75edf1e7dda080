"""CPU-side checks of the boundary of the world objects (include/sdm.h: sdm_world_objects_update / sdm_get_world_objects /
sdm_get_world_object_cells / sdm_get_world_object_labels / sdm_query_world_objects): the symbols are declared, exported
and bound with their signatures, the four structs have the sizes, fields and offsets the header gives them, the flag bits
are distinct and agree with the header, the header's bytes per brick, cell and object are what the layer keeps, and every
call is refused without a map."""
import ctypes as C
import inspect

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_objects_update", "sdm_get_world_objects", "sdm_get_world_object_cells", "sdm_get_world_object_labels",
         "sdm_query_world_objects")


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [2, 5, 7, 3, 6])))
    assert L.sdm_get_world_objects.argtypes[2:4] == [C.c_int32, C.POINTER(C.c_int32)]
    assert L.sdm_get_world_object_cells.argtypes[4:7] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert L.sdm_query_world_objects.argtypes[3] == C.c_int64 and L.sdm_query_world_objects.argtypes[5] == C.c_uint32
    want = dict(world_objects_update=["face_connected", "by_track", "static_only", "movable_only", "observed_only", "labels", "box", "min_cells",
                                      "max_cells"],
                world_objects=[], world_object_cells=["first", "cap"], world_object_labels=[], world_object_members=["i"],
                query_world_objects=["xyz", "cells", "on_device", "n", "out"])
    for f, args in want.items():
        assert list(inspect.signature(getattr(binding.SdmMap, f)).parameters)[1:] == args, f
    sig = inspect.signature(binding.SdmMap.world_objects_update).parameters
    assert [sig[k].default for k in want["world_objects_update"]] == [False, False, False, False, False, binding.ALL_LABELS, None, 1, 0]
    assert inspect.signature(binding.SdmMap.query_world_objects).parameters.keys() == inspect.signature(binding.SdmMap.query_world_distance).parameters.keys()


def test_struct_sizes_fields_and_offsets():
    dtypes = dict(sdm_world_objects_options=binding.WORLD_OBJECTS_OPTIONS, sdm_world_object=binding.WORLD_OBJECT,
                  sdm_world_objects_info=binding.WORLD_OBJECTS_INFO, sdm_world_object_result=binding.WORLD_OBJECT_RESULT)
    sizes = dict(sdm_world_objects_options=72, sdm_world_object=168, sdm_world_objects_info=40, sdm_world_object_result=24)
    for name, size in sizes.items():
        assert_layout(dtypes[name], name, size)
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_OBJECTS_OPTIONS) == dict(flags=0, min_cells=4, max_cells=8, labels=16, bmin=48, bmax=60)
    assert offsets(binding.WORLD_OBJECT) == dict(first_index=0, n_cells=4, n_guessed=8, track=12, label=14, mixed_tracks=15, first_cell=16,
                                                 cell_min=28, cell_max=40, pad0=52, cell_sum=56, cell_sq=80, box_min=128, box_max=140,
                                                 centroid=152, pad1=164)
    assert offsets(binding.WORLD_OBJECTS_INFO) == dict(n_bricks=0, n_objects=4, n_objects_total=8, flags=12, n_cells=16, n_guessed=24,
                                                       min_cells=32, stamp=36)
    assert offsets(binding.WORLD_OBJECT_RESULT) == dict(cell=0, object=12, index=16, pad=20)
    t = binding.WORLD_OBJECT
    assert t.fields["first_cell"][0].base == np.dtype("<i4") and t.fields["cell_sum"][0].base == np.dtype("<i8") and t.fields["cell_sq"][0].shape == (6,)
    assert t.fields["track"][0] == np.dtype("<u2") and t.fields["label"][0] == np.dtype("u1") and t.fields["mixed_tracks"][0] == np.dtype("u1")
    assert all(t.fields[f][0].shape == (3,) for f in ("first_cell", "cell_min", "cell_max", "cell_sum", "box_min", "box_max", "centroid"))
    o = binding.WORLD_OBJECTS_OPTIONS
    assert o.fields["max_cells"][0] == np.dtype("<i8") and o.fields["min_cells"][0] == np.dtype("<i4") and o.fields["labels"][0].shape == (8,)


def test_flag_bits_and_the_stated_bytes():
    names = ("FACE_CONNECTED", "BOX", "BY_TRACK", "STATIC_ONLY", "MOVABLE_ONLY", "OBSERVED_ONLY")
    bits = [define("SDM_WORLD_OBJECTS_" + n) for n in names]
    assert bits == [getattr(binding, "WORLD_OBJECTS_" + n) for n in names] == [1, 2, 4, 8, 16, 32]
    assert define("SDM_WORLD_OBJECT_UNLISTED") == binding.WORLD_OBJECT_UNLISTED == 0xFFFFFFFE
    assert define("SDM_WORLD_OBJECT_NONE") == binding.WORLD_OBJECT_NONE == 0xFFFFFFFF
    # per archived brick: flag, rank; per brick: coordinates, pool slot, 27 neighbours, counted words, prefix, two hash slots
    assert define("SDM_WORLD_OBJECTS_BYTES_PER_ARCHIVED_BRICK") == binding.WORLD_OBJECTS_BYTES_PER_ARCHIVED_BRICK == 4 + 4
    assert define("SDM_WORLD_OBJECTS_BYTES_PER_BRICK") == binding.WORLD_OBJECTS_BYTES_PER_BRICK == 8 + 4 + 27 * 4 + 8 * 8 + 8 * 4 + 2 * (8 + 4)
    # per cell: world cell, word, object, root, scan - within the 32 bytes the layer was given
    assert define("SDM_WORLD_OBJECTS_BYTES_PER_CELL") == binding.WORLD_OBJECTS_BYTES_PER_CELL == 12 + 4 + 3 * 4 <= 32
    # per object: the table entry, the accumulator (3 sums, 6 products, 2 counts, 6 box codes, the OR and a pad), first cell, scan
    acc = 3 * 8 + 6 * 8 + 2 * 4 + 6 * 4 + 4 + 4
    assert define("SDM_WORLD_OBJECTS_BYTES_PER_OBJECT") == binding.WORLD_OBJECTS_BYTES_PER_OBJECT == binding.WORLD_OBJECT.itemsize + acc + 4 + 4
    assert binding.label_mask(binding.ALL_LABELS).tolist() == [0xFFFFFFFF] * 8


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_OBJECTS_OPTIONS), np.zeros(1, binding.WORLD_OBJECTS_INFO)
    out, res, cell = np.zeros(2, binding.WORLD_OBJECT), np.zeros(2, binding.WORLD_OBJECT_RESULT), np.zeros((2, 3), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n32, n64 = C.c_int32(-7), C.c_int64(-7)
    assert L.sdm_world_objects_update(None, vp(o)) == INV
    assert L.sdm_get_world_objects(None, vp(out), 2, C.byref(n32), vp(info)) == INV and n32.value == -7
    assert L.sdm_get_world_object_cells(None, None, None, None, 0, 0, C.byref(n64)) == INV and n64.value == -7
    assert L.sdm_get_world_object_labels(None, None, None) == INV
    assert L.sdm_query_world_objects(None, None, vp(cell), 2, vp(res), 0) == INV
