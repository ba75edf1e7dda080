"""CPU-side checks of the boundary of the world mesh (include/sdm.h: sdm_world_mesh_update / sdm_get_world_mesh_info /
sdm_get_world_mesh_faces / sdm_get_world_mesh_vertices / sdm_world_mesh_device): the symbols are declared, exported and
bound with their signatures, the three structs have the sizes, fields and offsets the header gives them, the flag bits are
distinct and agree with the header, the header's bytes are the stated sums, and every call is refused without a map."""
import ctypes as C
import inspect

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_mesh_update", "sdm_get_world_mesh_info", "sdm_get_world_mesh_faces", "sdm_get_world_mesh_vertices", "sdm_world_mesh_device")


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [2, 2, 7, 6, 4])))
    assert L.sdm_get_world_mesh_faces.argtypes[4:7] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert L.sdm_get_world_mesh_vertices.argtypes[3:6] == [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert L.sdm_world_mesh_device.argtypes[1:] == [C.POINTER(C.c_void_p)] * 3
    update = ["labels", "track", "static_only", "movable_only", "observed_only", "skip_unknown_faces", "skip_absent_faces", "box", "max_faces",
              "max_vertices"]
    sig = inspect.signature(binding.SdmMap.world_mesh_update).parameters
    assert list(sig)[1:] == update and [sig[k].default for k in update] == [None, -1, False, False, False, False, False, None, 0, 0]
    for f in ("world_mesh_info", "world_mesh", "world_mesh_device"):
        assert list(inspect.signature(getattr(binding.SdmMap, f)).parameters) == ["self"], f
    assert list(inspect.signature(binding.SdmMap.save_world_ply).parameters) == ["self", "path", "update_kwargs"]


def test_struct_sizes_fields_and_offsets():
    dtypes = dict(sdm_world_mesh_options=(binding.WORLD_MESH_OPTIONS, 80), sdm_world_mesh_face=(binding.WORLD_MESH_FACE, 12),
                  sdm_world_mesh_info=(binding.WORLD_MESH_INFO, 200))
    for name, (dt, size) in dtypes.items():
        assert_layout(dt, name, size)
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_MESH_OPTIONS) == dict(flags=0, track=4, labels=8, bmin=40, bmax=52, max_faces=64, max_vertices=72)
    assert offsets(binding.WORLD_MESH_FACE) == dict(brick=0, cell=4, dir=6, kind=7, track=8, label=10, occ=11)
    assert offsets(binding.WORLD_MESH_INFO) == dict(n_bricks=0, n_vertex_bricks=4, n_faces=8, n_vertices=16, n_solid=24, faces_by_dir=32,
                                                    faces_by_kind=80, stamp=112, pad=116, options=120)
    f, i = binding.WORLD_MESH_FACE, binding.WORLD_MESH_INFO
    assert f.fields["brick"][0] == np.dtype("<u4") and f.fields["cell"][0] == np.dtype("<u2") and f.fields["occ"][0] == np.dtype("i1")
    assert i.fields["faces_by_dir"][0].shape == (6,) and i.fields["faces_by_kind"][0].shape == (4,) and i.fields["n_faces"][0] == np.dtype("<i8")
    assert i.fields["options"][0] == binding.WORLD_MESH_OPTIONS


def test_flag_bits_constants_and_the_stated_bytes():
    flags = ("STATIC_ONLY", "MOVABLE_ONLY", "OBSERVED_ONLY", "SKIP_UNKNOWN_FACES", "SKIP_ABSENT_FACES", "BOX")
    assert [define("SDM_WORLD_MESH_" + f) for f in flags] == [getattr(binding, "WORLD_MESH_" + f) for f in flags] == [1, 2, 4, 8, 16, 32]
    # the solid rule's bits are the block mesh's
    assert [binding.WORLD_MESH_STATIC_ONLY, binding.WORLD_MESH_MOVABLE_ONLY, binding.WORLD_MESH_OBSERVED_ONLY, binding.WORLD_MESH_SKIP_UNKNOWN_FACES] == \
        [binding.MESH_STATIC_ONLY, binding.MESH_MOVABLE_ONLY, binding.MESH_OBSERVED_ONLY, binding.MESH_SKIP_UNKNOWN_FACES]
    for name in ("ARCHIVED_BRICK", "BRICK", "VERTEX_SLOT", "VERTEX_BRICK", "FACE", "VERTEX"):
        assert define("SDM_WORLD_MESH_BYTES_PER_" + name) == getattr(binding, "WORLD_MESH_BYTES_PER_" + name), name
    assert binding.WORLD_MESH_BYTES_PER_ARCHIVED_BRICK == 4 + 4 + 3 * 8 * 8          # box flag, rank, three masks of eight words
    assert binding.WORLD_MESH_BYTES_PER_BRICK == 8 + 4 + 6 * 4 + 2 * 8 * 4 + 8 * 4   # coordinates, slot, neighbours, owners twice, prefix
    assert binding.WORLD_MESH_BYTES_PER_VERTEX_SLOT == 8 + 4 + 4 + 512 // 8          # key, rank, place in the list, 512 corner bits
    assert binding.WORLD_MESH_BYTES_PER_VERTEX_BRICK == 4 * 4 + 8 * 4                # the sort's four words, eight levels' prefix
    assert binding.WORLD_MESH_BYTES_PER_FACE == binding.WORLD_MESH_FACE.itemsize + 4 * 4 and binding.WORLD_MESH_BYTES_PER_VERTEX == 3 * 4
    assert 3 * 17 <= 64 and 32768 + 32768 < 1 << 17                                  # what a vertex brick's key has to hold


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, info = np.zeros(1, binding.WORLD_MESH_OPTIONS), np.zeros(1, binding.WORLD_MESH_INFO)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n64 = C.c_int64(-7)
    p = C.c_void_p(5)
    assert L.sdm_world_mesh_update(None, vp(o)) == INV
    assert L.sdm_get_world_mesh_info(None, vp(info)) == INV
    assert L.sdm_get_world_mesh_faces(None, None, None, None, 0, 0, C.byref(n64)) == INV and n64.value == -7
    assert L.sdm_get_world_mesh_vertices(None, None, None, 0, 0, C.byref(n64)) == INV and n64.value == -7
    assert L.sdm_world_mesh_device(None, C.byref(p), None, None) == INV and p.value == 5
