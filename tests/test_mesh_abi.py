"""CPU-side checks of the surface mesh's boundary (include/sdm.h: sdm_mesh_update / sdm_get_mesh_info / sdm_get_mesh_faces /
sdm_get_mesh_vertices / sdm_mesh_device): the symbols are declared, exported and bound, the structs have the sizes and
fields the header gives them, the constants agree with the header, and every call is refused without a map."""
import ctypes as C

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_mesh_update", "sdm_get_mesh_info", "sdm_get_mesh_faces", "sdm_get_mesh_vertices", "sdm_mesh_device")


def test_symbols_are_declared_exported_and_bound():
    assert_bound(dict(zip(NAMES, [2, 3, 5, 5, 4])))
    for f in ("mesh_update", "mesh", "mesh_info", "mesh_device"):
        assert callable(getattr(binding.SdmMap, f)), f
    assert callable(binding.mesh_triangles) and callable(binding.write_ply)


def test_struct_sizes_and_fields():
    sizes = dict(sdm_mesh_options=56, sdm_mesh_face=12, sdm_mesh_vertex=8, sdm_mesh_info=112)
    dtypes = dict(sdm_mesh_options=binding.MESH_OPTIONS, sdm_mesh_face=binding.MESH_FACE, sdm_mesh_vertex=binding.MESH_VERTEX,
                  sdm_mesh_info=binding.MESH_INFO)
    for name, size in sizes.items():
        assert_layout(dtypes[name], name, size)
    assert binding.MESH_INFO.fields["options"][0] == binding.MESH_OPTIONS and binding.MESH_INFO.fields["options"][1] % 8 == 0
    assert binding.MESH_OPTIONS.fields["max_faces"][1] % 8 == 0


def test_constants_agree_with_the_header():
    assert define("SDM_MESH_STATIC_ONLY") == binding.MESH_STATIC_ONLY == 0x01
    assert define("SDM_MESH_MOVABLE_ONLY") == binding.MESH_MOVABLE_ONLY == 0x02
    assert define("SDM_MESH_OBSERVED_ONLY") == binding.MESH_OBSERVED_ONLY == 0x04
    assert define("SDM_MESH_SKIP_UNKNOWN_FACES") == binding.MESH_SKIP_UNKNOWN_FACES == 0x08
    assert define("SDM_MESH_SKIP_BORDER_FACES") == binding.MESH_SKIP_BORDER_FACES == 0x10
    assert define("SDM_MESH_BYTES_PER_FACE") == binding.MESH_FACE.itemsize + 16 == 28
    assert define("SDM_MESH_BYTES_PER_VERTEX") == binding.MESH_VERTEX.itemsize == 8
    assert define("SDM_MESH_BYTES_PER_WORD") == 3 * 8 + 4 and define("SDM_MESH_BYTES_PER_CORNER_WORD") == 8 + 4


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info, origin = np.zeros(1, binding.MESH_OPTIONS), np.zeros(1, binding.MESH_INFO), np.zeros(3, np.float32)
    faces, quads = np.zeros(4, binding.MESH_FACE), np.zeros((4, 4), np.uint32)
    corners, xyz = np.zeros(4, binding.MESH_VERTEX), np.zeros((4, 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = C.c_int64(-7)
    p = [C.c_void_p(5) for _ in range(3)]
    assert L.sdm_mesh_update(None, None) == INV and L.sdm_mesh_update(None, vp(o)) == INV
    assert L.sdm_get_mesh_info(None, None, None) == INV and L.sdm_get_mesh_info(None, vp(info), vp(origin)) == INV
    assert L.sdm_get_mesh_faces(None, None, None, 0, None) == INV and L.sdm_get_mesh_faces(None, vp(faces), vp(quads), 4, C.byref(n)) == INV
    assert L.sdm_get_mesh_vertices(None, None, None, 0, None) == INV and L.sdm_get_mesh_vertices(None, vp(corners), vp(xyz), 4, C.byref(n)) == INV
    assert L.sdm_mesh_device(None, None, None, None) == INV and L.sdm_mesh_device(None, *(C.byref(x) for x in p)) == INV
    assert n.value == -7 and [x.value for x in p] == [5, 5, 5] and not info.view(np.uint8).any()   # nothing was written
