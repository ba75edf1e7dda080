"""CPU-side checks of the boundary of the world frontiers (include/sdm.h: sdm_world_frontiers_update /
sdm_get_world_frontier_clusters / sdm_get_world_frontier_cells): the symbols are declared, exported and bound with their
signatures, the three structs have the sizes, fields and offsets the header gives them, the flag bits are distinct and
agree with the header, the header's bytes per brick and per cell are the binding's dtypes', and every call is refused
without a map."""
import ctypes as C
import inspect

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_frontiers_update", "sdm_get_world_frontier_clusters", "sdm_get_world_frontier_cells")


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [2, 5, 7])))
    assert L.sdm_get_world_frontier_clusters.argtypes[2:4] == [C.c_int32, C.POINTER(C.c_int32)]
    assert L.sdm_get_world_frontier_cells.argtypes[4:7] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    want = dict(world_frontiers_update=["face_connected", "box", "inside_bricks", "min_cells", "max_cells"], world_frontiers=[],
                world_frontier_cells=["first", "cap"])
    for f, args in want.items():
        assert list(inspect.signature(getattr(binding.SdmMap, f)).parameters)[1:] == args, f
    sig = inspect.signature(binding.SdmMap.world_frontiers_update).parameters
    assert [sig[k].default for k in want["world_frontiers_update"]] == [False, None, False, 1, 0]


def test_struct_sizes_fields_and_offsets():
    dtypes = dict(sdm_world_frontiers_options=binding.WORLD_FRONTIERS_OPTIONS, sdm_world_frontier_cluster=binding.WORLD_FRONTIER_CLUSTER,
                  sdm_world_frontiers_info=binding.WORLD_FRONTIERS_INFO)
    sizes = dict(sdm_world_frontiers_options=40, sdm_world_frontier_cluster=120, sdm_world_frontiers_info=48)
    for name, size in sizes.items():
        assert_layout(dtypes[name], name, size)
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_FRONTIERS_OPTIONS) == dict(flags=0, min_cells=4, max_cells=8, bmin=16, bmax=28)
    assert offsets(binding.WORLD_FRONTIER_CLUSTER) == dict(first_index=0, n_cells=4, n_unknown_faces=8, pad0=12, first_cell=16, cell_min=28,
                                                            cell_max=40, pad1=52, cell_sum=56, box_min=80, box_max=92, centroid=104, pad2=116)
    assert offsets(binding.WORLD_FRONTIERS_INFO) == dict(n_bricks=0, n_clusters=4, n_clusters_total=8, flags=12, n_cells=16, n_unknown_faces=24,
                                                         n_absent_faces=32, min_cells=40, stamp=44)
    t = binding.WORLD_FRONTIER_CLUSTER
    assert t.fields["first_cell"][0].base == np.dtype("<i4") and t.fields["cell_sum"][0].base == np.dtype("<i8")
    assert all(t.fields[f][0].shape == (3,) for f in ("first_cell", "cell_min", "cell_max", "cell_sum", "box_min", "box_max", "centroid"))
    assert binding.WORLD_FRONTIERS_OPTIONS.fields["max_cells"][0] == np.dtype("<i8") and binding.WORLD_FRONTIERS_OPTIONS.fields["min_cells"][0] == np.dtype("<i4")


def test_flag_bits_and_the_stated_bytes():
    bits = [define("SDM_WORLD_FRONTIERS_FACE_CONNECTED"), define("SDM_WORLD_FRONTIERS_BOX"), define("SDM_WORLD_FRONTIERS_INSIDE_BRICKS")]
    assert bits == [binding.WORLD_FRONTIERS_FACE_CONNECTED, binding.WORLD_FRONTIERS_BOX, binding.WORLD_FRONTIERS_INSIDE_BRICKS] == [1, 2, 4]
    assert binding.WORLD_FRONTIER_NO_CLUSTER == 0xFFFFFFFF
    # per cell: accumulator (56), table entry, world cell, parent / root / scan words, unknown_faces
    assert define("SDM_WORLD_FRONTIERS_BYTES_PER_CELL") == 56 + binding.WORLD_FRONTIER_CLUSTER.itemsize + 12 + 3 * 4 + 1
    assert define("SDM_WORLD_FRONTIERS_BYTES_PER_BRICK") == 8 + 4 + 27 * 4 + 6 * 4 + 8 * 8 + 8 * 4
    assert define("SDM_WORLD_FRONTIERS_BYTES_PER_ARCHIVED_BRICK") == 4 + 4 + 2 * 64


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_FRONTIERS_OPTIONS), np.zeros(1, binding.WORLD_FRONTIERS_INFO)
    out = np.zeros(2, binding.WORLD_FRONTIER_CLUSTER)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n32, n64 = C.c_int32(-7), C.c_int64(-7)
    assert L.sdm_world_frontiers_update(None, vp(o)) == INV
    assert L.sdm_get_world_frontier_clusters(None, vp(out), 2, C.byref(n32), vp(info)) == INV and n32.value == -7
    assert L.sdm_get_world_frontier_cells(None, None, None, None, 0, 0, C.byref(n64)) == INV and n64.value == -7
