"""CPU-side checks of the forecast's boundary (include/sdm.h: sdm_forecast_stamps / sdm_forecast_update / sdm_get_forecast /
sdm_get_forecast_cells / sdm_query_forecast / sdm_query_forecast_segments): the symbols are declared, exported and bound,
the layouts and constants agree with the header, the calls that need a map are refused without one, and the stamp routine
- host code that needs no device - gives the stamps of tests/forecast_ref.py and refuses what the header says it refuses."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import forecast_ref as fc
from tests.abi_checks import assert_bound, assert_layout, define

NAMES = ("sdm_forecast_stamps", "sdm_forecast_update", "sdm_get_forecast", "sdm_get_forecast_cells", "sdm_query_forecast",
         "sdm_query_forecast_segments")
INV, CAPACITY = 1, 4
SIZE = 0.1


def test_symbols_are_declared_exported_and_bound():
    assert_bound(dict(zip(NAMES, [9, 6, 5, 6, 5, 5])))
    for f in ("forecast_update", "forecast", "forecast_cells", "query_forecast", "query_forecast_segments"):
        assert callable(getattr(binding.SdmMap, f)), f
    assert callable(binding.forecast_stamps)


def test_layouts_and_constants_agree_with_the_header():
    assert define("SDM_FORECAST_SWEPT") == binding.FORECAST_SWEPT == fc.SWEPT == 1
    assert define("SDM_FORECAST_VACATED_BLOCKS") == binding.FORECAST_VACATED_BLOCKS == 4
    assert binding.FORECAST_VACATED_BLOCKS & (binding.QUERY_ON_DEVICE | binding.QUERY_UNKNOWN_BLOCKS) == 0
    assert define("SDM_FORECAST_MAX_HORIZONS") == binding.FORECAST_MAX_HORIZONS == fc.MAX_HORIZONS == 16
    assert define("SDM_FORECAST_MAX_STAMPS") == binding.FORECAST_MAX_STAMPS == fc.MAX_STAMPS == 65536
    dtypes = dict(sdm_motion=(binding.MOTION, 16), sdm_forecast_stamp=(binding.FORECAST_STAMP, 12), sdm_forecast_info=(binding.FORECAST_INFO, 40),
                  sdm_forecast_result=(binding.FORECAST_RESULT, 8), sdm_forecast_hit=(binding.FORECAST_HIT, 16))
    for name, (dt, size) in dtypes.items():
        assert_layout(dt, name, size)
    assert binding.MOTION == fc.MOTION and binding.FORECAST_STAMP == fc.STAMP
    assert binding.FORECAST_INFO.names == ("n_motions", "n_horizons", "n_stamps", "flags", "n_sources", "n_marked", "n_marks_in", "n_marks_out")
    assert binding.FORECAST_INFO.fields["n_marks_in"][1] == 24


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    n = C.c_int64(0)
    assert L.sdm_forecast_update(None, None, 0, None, 0, 0) == INV
    assert L.sdm_get_forecast(None, None, None, None, None) == INV
    assert L.sdm_get_forecast_cells(None, None, None, None, 0, C.byref(n)) == INV
    assert L.sdm_query_forecast(None, None, 0, None, 0) == INV
    assert L.sdm_query_forecast_segments(None, None, 0, None, 0) == INV


def same(got, want):
    assert got.dtype == want.dtype and len(got) == len(want), (len(got), len(want))
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:4]


@pytest.mark.parametrize("swept", [False, True])
def test_stamps_of_random_motions(swept):
    rng = np.random.default_rng(11)
    for size in (0.1, 0.25, 0.3, 1.0):
        tracks = rng.choice(np.arange(1, 65536), 12, replace=False)
        mo = fc.motions(tracks, rng.normal(0, 3.0, (12, 3)))
        t = np.cumsum(rng.uniform(0.05, 0.6, 7)).astype(np.float32)
        same(binding.forecast_stamps(size, mo, t, swept), fc.stamps(size, mo, t, swept))
    assert (np.diff(fc.stamps(size, mo, t, swept)["track"].astype(np.int64)) >= 0).all()   # ascending track, whatever the motions' order


def test_ties_round_to_even_and_shifts_are_clamped():
    # v * t / size exactly x.5: in float64 with size = 0.25 and t = 1 every multiple of 0.125 is exact
    v = np.array([[0.125, -0.125, 0.375], [-0.375, 0.625, -0.625], [0.875, -0.875, 1.125]], np.float32)
    mo = fc.motions([7, 8, 9], v)
    got = binding.forecast_stamps(0.25, mo, [1.0])
    assert got["d"].tolist() == [[0, 0, 2], [-2, 2, -2], [4, -4, 4]]
    same(got, fc.stamps(0.25, mo, [1.0]))
    # nothing moves; the clamp at +-1024 cells, also for products far beyond an int
    big = fc.motions([1, 2, 3], [[0, 0, 0], [1e30, -1e30, 102.4], [3e38, -102.5, 102.45]])
    got = binding.forecast_stamps(SIZE, big, [1.0, 3e38])
    same(got, fc.stamps(SIZE, big, [1.0, 3e38]))
    assert got["d"][0].tolist() == [0, 0, 0] and got["d"][2].tolist() == [1024, -1024, 1024] and got["d"][3].tolist() == [1024, -1024, 1024]
    assert (np.abs(got["d"]) <= 1024).all() and (got["pad"] == 0).all() and (got["pad2"] == 0).all()


def test_swept_lines():
    one = np.float32(1.0)
    for d in ([6, 0, 0], [0, -5, 0], [4, 4, 0], [0, -3, 3], [3, 3, 3], [-4, 4, -4], [5, -2, 1], [0, 0, 0]):
        mo = fc.motions([3], [np.array(d, np.float32) * one])
        got = binding.forecast_stamps(1.0, mo, [1.0, 2.0], swept=True)
        same(got, fc.stamps(1.0, mo, [1.0, 2.0], swept=True))
        J = max(1, max(abs(x) for x in d))
        assert len(got) == 2 * J and got["horizon"].tolist() == [0] * J + [1] * J
        assert got["d"][J - 1].tolist() == d and got["d"][-1].tolist() == [2 * x for x in d]   # each horizon's line ends on its shift
    # (5, -2, 1): the line of the header's formula
    got = binding.forecast_stamps(1.0, fc.motions([3], [[5, -2, 1]]), [1.0], swept=True)
    assert got["d"].tolist() == [[1, 0, 0], [2, -1, 0], [3, -1, 1], [4, -2, 1], [5, -2, 1]]
    # J == 0 at a later horizon: the object has not moved a cell since the horizon before
    got = binding.forecast_stamps(1.0, fc.motions([3], [[1, 0, 0]]), [2.0, 2.25], swept=True)
    assert got["d"].tolist() == [[1, 0, 0], [2, 0, 0], [2, 0, 0]] and got["horizon"].tolist() == [0, 0, 1]


def test_the_stamp_cap():
    L = binding.load_library()
    n = C.c_int64(0)

    def count(mo, t, flags):
        tt = np.asarray(t, np.float32)
        return L.sdm_forecast_stamps(SIZE, binding._ptr(mo), len(mo), binding._ptr(tt), len(tt), flags, None, 0, C.byref(n)), n.value

    still = lambda k: fc.motions(np.arange(1, k + 1), np.zeros((k, 3)))  # noqa: E731
    t16, t15 = np.arange(1, 17), np.arange(1, 16)
    assert count(still(4369), t15, 0) == (0, 65535)
    assert count(still(4096), t16, 0) == (0, 65536)
    same(binding.forecast_stamps(SIZE, still(4096), t16), fc.stamps(SIZE, still(4096), t16))
    # one above: under SWEPT one of the 4096 moves two cells in its last interval and one in every other
    mo = still(4096)
    mo["v"][77] = [np.float32(SIZE), 0, 0]
    t = np.concatenate([np.arange(1, 16), [17]])
    assert count(mo, t, 1) == (CAPACITY, 65537) and "65537" in L.sdm_last_error().decode()
    assert count(mo, t16, 1) == (0, 65536)
    # a capacity below the count: the first entries, nothing beyond them, the true count
    some, total = binding.forecast_stamps(SIZE, still(10), t16, cap=25)
    assert total == 160 and len(some) == 25
    same(some, fc.stamps(SIZE, still(10), t16)[:25])
    guard = np.full(30, 0x5A, binding.FORECAST_STAMP)
    tt = t16.astype(np.float32)
    assert L.sdm_forecast_stamps(SIZE, binding._ptr(still(10)), 10, binding._ptr(tt), 16, 0, binding._ptr(guard), 25, C.byref(n)) == 0
    assert guard[25:].tobytes() == np.full(5, 0x5A, binding.FORECAST_STAMP).tobytes()


def test_refusals():
    L = binding.load_library()
    n = C.c_int64(0)
    out = np.zeros(64, binding.FORECAST_STAMP)

    def call(mo, t, flags=0, size=SIZE, n_mo=None, n_t=None):
        tt = np.asarray(t, np.float32)
        return L.sdm_forecast_stamps(size, binding._ptr(mo) if mo is not None else None, len(mo) if n_mo is None else n_mo,
                                     binding._ptr(tt), len(tt) if n_t is None else n_t, flags, binding._ptr(out), len(out), C.byref(n))

    ok = fc.motions([4, 9], [[1, 0, 0], [0, 1, 0]])
    assert call(ok, [0.5, 1.0]) == 0 and n.value == 4
    assert call(None, [0.5], n_mo=0) == 0 and n.value == 0                       # no motions: allowed
    assert call(fc.motions([4, 9, 4], np.zeros((3, 3))), [0.5]) == INV and "twice" in L.sdm_last_error().decode()
    assert call(fc.motions([0], np.zeros((1, 3))), [0.5]) == INV
    for bad in (np.nan, np.inf, -np.inf):
        mo = fc.motions([4], [[0, bad, 0]])
        assert call(mo, [0.5]) == INV
    mo = fc.motions([4], np.zeros((1, 3)))
    mo["pad"] = 1
    assert call(mo, [0.5]) == INV
    for t in ([0.5, 0.5], [1.0, 0.5], [0.0, 1.0], [-1.0, 1.0], [0.5, np.nan], [0.5, np.inf]):
        assert call(ok, t) == INV, t
    assert call(ok, np.arange(1, 18)) == INV and call(ok, [1.0], n_t=0) == INV    # 17 horizons, none
    assert call(ok, np.arange(1, 17)) == 0
    for flags in (0x2, 0x4, 0x80000000):
        assert call(ok, [0.5], flags=flags) == INV
    assert call(ok, [0.5], n_mo=-1) == INV and call(None, [0.5], n_mo=2) == INV
    for size in (0.0, -0.1, np.nan):
        assert call(ok, [0.5], size=size) == INV
    assert L.sdm_forecast_stamps(SIZE, binding._ptr(ok), 2, binding._ptr(np.ones(1, np.float32)), 1, 0, None, 4, C.byref(n)) == INV   # no out
    assert L.sdm_forecast_stamps(SIZE, binding._ptr(ok), 2, binding._ptr(np.ones(1, np.float32)), 1, 0, binding._ptr(out), 4, None) == INV
