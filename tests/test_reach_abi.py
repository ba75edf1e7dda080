"""CPU-side checks of the travel-cost boundary (include/sdm.h: sdm_reach_update / sdm_get_reach / sdm_query_reach /
sdm_reach_paths): the symbols are declared, exported and bound, the constants agree with the header, and the calls
that need no device are refused as the header says."""
import ctypes as C

from semantic_dsp_map_amd import binding
from tests.abi_checks import assert_bound, define

NAMES = ("sdm_reach_update", "sdm_get_reach", "sdm_query_reach", "sdm_reach_paths", "sdm_debug_reach_tiles")


def test_symbols_are_declared_exported_and_bound():
    assert_bound(dict(zip(NAMES, [7, 4, 6, 8, 2])))
    for f in ("reach_update", "reach", "query_reach", "reach_paths"):
        assert callable(getattr(binding.SdmMap, f)), f


def test_constants_agree_with_the_header():
    assert define("SDM_REACH_FACE_CONNECTED") == binding.REACH_FACE_CONNECTED == 1
    assert define("SDM_REACH_THROUGH_UNKNOWN") == binding.REACH_THROUGH_UNKNOWN == 2
    assert define("SDM_REACH_COST_PER_CELL") == binding.REACH_COST_PER_CELL == 10
    assert binding.REACH_INFO.names == ("n_starts_used", "n_traversable", "n_reached", "max_cost_reached", "rounds", "flags", "min_d2", "max_cost")


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    INV = 1
    n = C.c_int64(0)
    assert L.sdm_reach_update(None, None, None, 0, 0, 0, 0) == INV
    assert L.sdm_get_reach(None, None, None, None) == INV
    assert L.sdm_query_reach(None, None, None, 0, None, 0) == INV
    assert L.sdm_reach_paths(None, None, None, 0, 0, None, None, 0) == INV
    assert L.sdm_debug_reach_tiles(None, C.byref(n)) == INV
