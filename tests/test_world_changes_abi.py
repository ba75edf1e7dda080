"""CPU-side checks of the boundary of the world changes (include/sdm.h: sdm_world_changes_update / sdm_get_world_changes /
sdm_get_world_change_cells / sdm_get_world_change_labels / sdm_query_world_changes): the symbols are declared, exported and
bound with their signatures, the four structs have the sizes, fields and offsets the header gives them, the flag bits and
classes are distinct and agree with the header, the header's bytes per candidate, brick, cell and region are what the layer
keeps, and every call is refused without a map."""
import ctypes as C
import inspect

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_changes_update", "sdm_get_world_changes", "sdm_get_world_change_cells", "sdm_get_world_change_labels",
         "sdm_query_world_changes")


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [2, 5, 9, 4, 6])))
    assert L.sdm_get_world_changes.argtypes[2:4] == [C.c_int32, C.POINTER(C.c_int32)]
    assert L.sdm_get_world_change_cells.argtypes[6:9] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert L.sdm_query_world_changes.argtypes[3] == C.c_int64 and L.sdm_query_world_changes.argtypes[5] == C.c_uint32
    want = dict(update=["face_connected", "by_label", "static_only", "observed_only", "max_last_stamp", "labels", "classes", "min_cells", "max_cells"],
                regions=[], cells=["first", "cap"], labels=[], query=["xyz", "cells", "on_device", "n", "out"])
    for f, args in want.items():
        assert list(inspect.signature(getattr(binding.WorldChanges, f)).parameters)[1:] == args, f
    sig = inspect.signature(binding.WorldChanges.update).parameters
    assert [sig[k].default for k in want["update"]] == [False, False, False, False, None, binding.ALL_LABELS, binding.ALL_CHANGE_CLASSES, 1, 0]
    assert inspect.signature(binding.WorldChanges.query).parameters.keys() == inspect.signature(binding.SdmMap.query_world_objects).parameters.keys()
    assert not issubclass(binding.SdmMap, binding.WorldChanges) and not any(n.startswith("world_change") for n in vars(binding.SdmMap))


def test_struct_sizes_fields_and_offsets():
    dtypes = dict(sdm_world_changes_options=binding.WORLD_CHANGES_OPTIONS, sdm_world_change_region=binding.WORLD_CHANGE_REGION,
                  sdm_world_changes_info=binding.WORLD_CHANGES_INFO, sdm_world_change_result=binding.WORLD_CHANGE_RESULT)
    sizes = dict(sdm_world_changes_options=64, sdm_world_change_region=112, sdm_world_changes_info=128, sdm_world_change_result=24)
    for name, size in sizes.items():
        assert_layout(dtypes[name], name, size)
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_CHANGES_OPTIONS) == dict(flags=0, min_cells=4, max_cells=8, labels=16, classes=48, max_last_stamp=52, pad=56)
    assert offsets(binding.WORLD_CHANGE_REGION) == dict(first_index=0, n_cells=4, cls=8, label_now=9, label_before=10, mixed=11, first_cell=12,
                                                        cell_min=24, cell_max=36, cell_sum=48, box_min=72, box_max=84, centroid=96, pad=108)
    info = offsets(binding.WORLD_CHANGES_INFO)
    assert [info[n] for n in binding.WORLD_CHANGES_COUNTERS] == list(range(0, 88, 8)) and len(binding.WORLD_CHANGES_COUNTERS) == 11
    assert all(binding.WORLD_CHANGES_INFO.fields[n][0] == np.dtype("<u8") for n in binding.WORLD_CHANGES_COUNTERS)
    assert {k: v for k, v in info.items() if v >= 88} == dict(n_candidates=88, n_bricks=92, n_cells=96, n_regions=104, n_regions_total=108,
                                                              flags=112, min_cells=116, frame_stamp=120, stamp=124)
    assert offsets(binding.WORLD_CHANGE_RESULT) == dict(cell=0, region=12, index=16, cls=20)
    t = binding.WORLD_CHANGE_REGION
    assert t.fields["first_cell"][0].base == np.dtype("<i4") and t.fields["cell_sum"][0].base == np.dtype("<i8")
    assert all(t.fields[f][0] == np.dtype("u1") for f in ("cls", "label_now", "label_before", "mixed"))
    assert all(t.fields[f][0].shape == (3,) for f in ("first_cell", "cell_min", "cell_max", "cell_sum", "box_min", "box_max", "centroid"))
    o = binding.WORLD_CHANGES_OPTIONS
    assert o.fields["max_cells"][0] == np.dtype("<i8") and o.fields["min_cells"][0] == np.dtype("<i4") and o.fields["labels"][0].shape == (8,)


def test_flag_bits_classes_and_the_stated_bytes():
    names = ("FACE_CONNECTED", "BY_LABEL", "STATIC_ONLY", "OBSERVED_ONLY", "OLDER")
    bits = [define("SDM_WORLD_CHANGES_" + n) for n in names]
    assert bits == [getattr(binding, "WORLD_CHANGES_" + n) for n in names] == [1, 2, 4, 8, 16]
    classes = [define("SDM_WORLD_CHANGE_" + n) for n in ("APPEARED", "VANISHED", "RELABELLED")]
    assert classes == list(binding.ALL_CHANGE_CLASSES) == [1, 2, 3]
    assert define("SDM_WORLD_CHANGE_UNLISTED") == binding.WORLD_CHANGE_UNLISTED == 0xFFFFFFFE
    assert define("SDM_WORLD_CHANGE_NONE") == binding.WORLD_CHANGE_NONE == 0xFFFFFFFF
    # per candidate: flag, rank, pool slot, the listed words and the two class planes
    assert define("SDM_WORLD_CHANGES_BYTES_PER_CANDIDATE") == binding.WORLD_CHANGES_BYTES_PER_CANDIDATE == 3 * 4 + 3 * 8 * 8
    # per brick: coordinates, pool slot, 27 neighbours, listed words, prefix, two class planes, two hash slots
    assert define("SDM_WORLD_CHANGES_BYTES_PER_BRICK") == binding.WORLD_CHANGES_BYTES_PER_BRICK == 8 + 4 + 27 * 4 + 8 * 8 + 8 * 4 + 2 * 8 * 8 + 2 * (8 + 4)
    # per cell: world cell, now, before, key, class, region, root, scan
    assert define("SDM_WORLD_CHANGES_BYTES_PER_CELL") == binding.WORLD_CHANGES_BYTES_PER_CELL == 12 + 3 * 4 + 1 + 3 * 4
    # per region: the table entry, the accumulator (3 sums, the count, 6 box codes, the OR), first cell, scan
    acc = 3 * 8 + 4 + 6 * 4 + 4
    assert define("SDM_WORLD_CHANGES_BYTES_PER_REGION") == binding.WORLD_CHANGES_BYTES_PER_REGION == binding.WORLD_CHANGE_REGION.itemsize + acc + 4 + 4


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_CHANGES_OPTIONS), np.zeros(1, binding.WORLD_CHANGES_INFO)
    out, res, cell = np.zeros(2, binding.WORLD_CHANGE_REGION), np.zeros(2, binding.WORLD_CHANGE_RESULT), np.zeros((2, 3), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n32, n64 = C.c_int32(-7), C.c_int64(-7)
    assert L.sdm_world_changes_update(None, vp(o)) == INV
    assert L.sdm_get_world_changes(None, vp(out), 2, C.byref(n32), vp(info)) == INV and n32.value == -7
    assert L.sdm_get_world_change_cells(None, None, None, None, None, None, 0, 0, C.byref(n64)) == INV and n64.value == -7
    assert L.sdm_get_world_change_labels(None, None, None, None) == INV
    assert L.sdm_query_world_changes(None, None, vp(cell), 2, vp(res), 0) == INV
