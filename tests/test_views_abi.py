"""CPU-side checks of the view-scoring boundary (include/sdm.h: sdm_query_views): the record layouts ctypes and numpy
see, the exported and bound symbols, and the ray table of a pinhole camera."""

import numpy as np

from semantic_dsp_map_amd import binding, synth
from tests.abi_checks import assert_bound, assert_layout


def test_layouts():
    assert_layout(binding.VIEW, "sdm_view", 32)
    assert_layout(binding.VIEW_GAIN, "sdm_view_gain", 40)
    assert [binding.VIEW.fields[k][1] for k in ("pos", "q", "range")] == [0, 12, 28]
    off = {k: binding.VIEW_GAIN.fields[k][1] for k in binding.VIEW_GAIN.names}
    assert off == dict(n_unknown=0, n_free=4, n_occupied=8, rays_hit=12, rays_in_map=16, pad=20, ray_cells=24, ray_unknown=32)
    assert binding.VIEW_MAX_RAYS == 65536


def test_symbols_are_declared_exported_and_bound():
    assert_bound(dict(sdm_query_views=9, sdm_debug_view_batch=2))
    assert callable(binding.SdmMap.query_views) and callable(binding.SdmMap.set_view_batch)


def test_calls_without_a_map_are_refused():
    L = binding.load_library()
    assert L.sdm_query_views(None, None, 0, None, 1, None, None, None, 0) == 1
    assert L.sdm_debug_view_batch(None, 3) == 1


def test_pinhole_rays():
    cfg = synth.CONFIGS["T0"]
    full = binding.pinhole_rays(cfg, 1)
    assert full.shape == (cfg["height"], cfg["width"], 3) and full.dtype == np.float32
    v, u = 7, 11
    want = ((np.float32(u) - np.float32(cfg["cx"])) / np.float32(cfg["fx"]), (np.float32(v) - np.float32(cfg["cy"])) / np.float32(cfg["fy"]), 1)
    assert tuple(full[v, u]) == want
    for stride in (2, 3, 8):
        assert np.array_equal(binding.pinhole_rays(cfg, stride), full[::stride, ::stride])
    c = binding.Config()
    for k, _ in binding.Config._fields_:
        if k in cfg:
            setattr(c, k, cfg[k])
    assert np.array_equal(binding.pinhole_rays(c, 4), full[::4, ::4])   # the structure a map holds, as well as the dictionary
