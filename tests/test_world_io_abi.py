"""CPU-side checks of the boundary of the world archive's import and retain (include/sdm.h: sdm_world_import /
sdm_world_retain): the symbols are declared, exported and bound, the option structs have the sizes, fields and offsets the
header gives them, the constants agree with the header and with each other, and both calls are refused without a map."""
import ctypes as C

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_world_import", "sdm_world_retain")


def test_symbols_are_declared_exported_and_bound():
    L = assert_bound(dict(zip(NAMES, [5, 3])))
    assert L.sdm_world_import.argtypes[4] is C.c_int64 and L.sdm_world_retain.argtypes[2] is C.POINTER(C.c_int64)
    for f in ("world_import", "world_retain", "save_world", "load_world"):
        assert callable(getattr(binding.SdmMap, f)), f


def test_struct_sizes_fields_and_offsets():
    sizes = dict(sdm_world_import_options=24, sdm_world_retain_options=32)
    dtypes = dict(sdm_world_import_options=binding.WORLD_IMPORT_OPTIONS, sdm_world_retain_options=binding.WORLD_RETAIN_OPTIONS)
    for name, size in sizes.items():
        assert_layout(dtypes[name], name, size)
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_IMPORT_OPTIONS) == dict(flags=0, cell_offset=4, max_bricks=16)
    assert offsets(binding.WORLD_RETAIN_OPTIONS) == dict(bmin=0, bmax=12, min_last_stamp=24, flags=28)
    assert binding.WORLD_IMPORT_OPTIONS.fields["cell_offset"][0].shape == (3,) and binding.WORLD_RETAIN_OPTIONS.fields["bmax"][0].shape == (3,)
    # the info an import reports through stays what it was
    assert binding.WORLD_INFO.itemsize == 80 and binding.WORLD_BRICK.itemsize == 20


def test_constants_agree_with_the_header():
    assert define("SDM_WORLD_IMPORT_FILL") == binding.WORLD_IMPORT_FILL == 0x10
    assert define("SDM_WORLD_IMPORT_ON_DEVICE") == binding.WORLD_IMPORT_ON_DEVICE
    bits = [define("SDM_WORLD_STATIC_ONLY"), define("SDM_WORLD_OBSERVED_ONLY"), define("SDM_WORLD_IMPORT_FILL"), define("SDM_WORLD_IMPORT_ON_DEVICE")]
    assert all(b and not b & (b - 1) for b in bits) and len(set(bits)) == 4     # four distinct bits share the import's flags word


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    o, r = np.zeros(1, binding.WORLD_IMPORT_OPTIONS), np.zeros(1, binding.WORLD_RETAIN_OPTIONS)
    bricks, cells = np.zeros(2, binding.WORLD_BRICK), np.zeros((2, 512), np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = C.c_int64(-7)
    assert L.sdm_world_import(None, None, None, None, 0) == INV and L.sdm_world_import(None, vp(o), vp(bricks), vp(cells), 2) == INV
    assert L.sdm_world_retain(None, None, None) == INV and L.sdm_world_retain(None, vp(r), C.byref(n)) == INV
    assert n.value == -7
