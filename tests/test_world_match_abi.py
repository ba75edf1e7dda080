"""CPU-side checks of the boundary of the world match (include/sdm.h: sdm_world_match): the symbol is declared, exported and
bound with its signature, the three structs have the sizes, fields and offsets the header gives them, the constants agree
with the header and with the import's, and the call is refused without a map."""
import ctypes as C
import re

import numpy as np

from semantic_dsp_map_amd import binding
from tests.abi_checks import HEADER, assert_bound, assert_layout, define

DTYPES = dict(sdm_world_match_options=binding.WORLD_MATCH_OPTIONS, sdm_world_match_score=binding.WORLD_MATCH_SCORE,
              sdm_world_match_result=binding.WORLD_MATCH_RESULT)


def test_the_symbol_is_declared_exported_and_bound():
    L = assert_bound(dict(sdm_world_match=7))
    vp = C.c_void_p
    assert L.sdm_world_match.argtypes == [vp, vp, vp, vp, C.c_int64, vp, vp]
    decl = re.search(r"sdm_status sdm_world_match\(([^;]*)\);", HEADER).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert [" ".join(a.split()) for a in decl.split(",")] == [
        "sdm_map *m", "const sdm_world_match_options *o", "const sdm_world_brick *bricks", "const uint32_t *cells", "int64_t n",
        "sdm_world_match_score *scores", "sdm_world_match_result *result"]
    for f in ("world_match", "world_align"):
        assert callable(getattr(binding.SdmMap, f)), f
    assert HEADER.index("sdm_status sdm_world_retain(") < HEADER.index("sdm_status sdm_world_match(") < HEADER.index("sdm_world_reach_update")


def test_struct_sizes_fields_and_offsets():
    sizes = dict(sdm_world_match_options=56, sdm_world_match_score=32, sdm_world_match_result=56)
    for name, size in sizes.items():
        assert_layout(DTYPES[name], name, size)
    offsets = lambda dt: {f: dt.fields[f][1] for f in dt.names}  # noqa: E731
    assert offsets(binding.WORLD_MATCH_OPTIONS) == dict(flags=0, cell_offset=4, radius=16, w_oo=28, w_same=32, w_of=36, w_fo=40, w_ff=44, pad=48)
    assert offsets(binding.WORLD_MATCH_SCORE) == dict(offset=0, n_oo=12, n_of=16, n_fo=20, n_ff=24, n_same=28)
    assert offsets(binding.WORLD_MATCH_RESULT) == dict(n_candidates=0, n_sources=4, src_occupied=8, src_free=12, best_score=16, runner_up=24,
                                                       best=32, best_offset=36, pad=48)
    for dt, f in ((binding.WORLD_MATCH_OPTIONS, "cell_offset"), (binding.WORLD_MATCH_OPTIONS, "radius"), (binding.WORLD_MATCH_SCORE, "offset"),
                  (binding.WORLD_MATCH_RESULT, "best_offset")):
        assert dt.fields[f][0].shape == (3,) and dt.fields[f][0].base == np.dtype("<i4")
    assert binding.WORLD_MATCH_RESULT.fields["best_score"][0] == np.dtype("<i8") == binding.WORLD_MATCH_RESULT.fields["runner_up"][0]


def test_constants_agree_with_the_header():
    assert define("SDM_WORLD_MATCH_ON_DEVICE") == binding.WORLD_MATCH_ON_DEVICE == define("SDM_WORLD_IMPORT_ON_DEVICE") == 0x20
    assert define("SDM_WORLD_MATCH_MAX_RADIUS") == binding.WORLD_MATCH_MAX_RADIUS == 8
    bits = [define("SDM_WORLD_STATIC_ONLY"), define("SDM_WORLD_OBSERVED_ONLY"), define("SDM_WORLD_MATCH_ON_DEVICE")]
    assert all(b and not b & (b - 1) for b in bits) and len(set(bits)) == 3
    assert tuple(binding.WORLD_MATCH_WEIGHTS) == (4, 1, -2, -2, 0)


def test_the_call_without_a_map_is_refused():
    L = binding.load_library()
    o, res = np.zeros(1, binding.WORLD_MATCH_OPTIONS), np.full(1, 7, binding.WORLD_MATCH_RESULT)
    bricks, cells = np.zeros(2, binding.WORLD_BRICK), np.zeros((2, 512), np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    before = res.tobytes()
    assert L.sdm_world_match(None, None, None, None, 0, None, None) == 1
    assert L.sdm_world_match(None, vp(o), vp(bricks), vp(cells), 2, None, vp(res)) == 1 and res.tobytes() == before
