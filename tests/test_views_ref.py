"""CPU checks of tests/views_ref.py, the NumPy restatement the GPU tests of sdm_query_views compare against: hand cases
whose answers can be read off the pattern, the float32 ray construction against shape_cases.quat_mat, and that
unambiguous_rays fills its table for the views the GPU tests use on every map shape."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import query_ref as qr
from tests import shape_cases as sc
from tests import views_ref as vr

RING = {"global_time_stamp": 3, "moved_steps": [5, -3, 9], "eq_steps": [5, 29, 9], "map_center": [1.0, -0.6, 1.8],
        "last_pos": [1.0, -0.6, 1.8], "birth_cursor": 0, "move_cursor": 0}
IDENTITY = (1.0, 0.0, 0.0, 0.0)


def _row_map():
    """T0's grid, every cell free but the x row (y, z) = (3, 5): cells 0..9 free, 10..14 unknown, 15 free, 16 occupied,
    17 unknown, the rest free"""
    cfg = synth.CONFIGS["T0"]
    geo = qr.Geometry(cfg, RING)
    vox = np.zeros(int(geo.N.prod()), binding.VOXEL_RESULT)
    row = np.array([[x, 3, 5] for x in range(int(geo.N[0]))], np.int64)
    v = geo.voxel(row)
    vox["occ"][v[10:15]] = -1
    vox["occ"][v[16]] = 1
    vox["occ"][v[17]] = -1
    return cfg, geo, vox, v


def _view(geo, u, q=IDENTITY, rng=1.0):
    size = np.float32(1) / geo.recip
    v = np.zeros(1, binding.VIEW)
    v["pos"] = (geo.center + geo.pmin + np.asarray(u, np.float32) * size).astype(np.float32)
    v["q"], v["range"] = q, rng
    return v


def test_one_ray_down_a_row():
    cfg, geo, vox, row = _row_map()
    size = float(cfg["voxel_size"])
    view = _view(geo, (2.5, 3.5, 5.5), rng=40 * size)   # 40 cells along +x: it would leave the map, the obstacle at 16 stops it
    gain, rays, unk = vr.query_views(geo, vox, view, [[1.0, 0.0, 0.0]])
    g = gain[0]
    assert (g["n_unknown"], g["n_free"], g["n_occupied"]) == (5, 9, 1)        # cells 2..16: 2..9 and 15 free, 10..14 unknown, 16 blocks
    assert (g["rays_hit"], g["rays_in_map"], g["ray_cells"], g["ray_unknown"], g["pad"]) == (1, 1, 15, 5, 0)
    assert rays["voxel"][0, 0] == row[16] and rays["cells"][0, 0] == 15 and rays["occ"][0, 0] == 1 and unk[0, 0] == 5
    assert abs(rays["t"][0, 0] - (16 - 2.5) / 40) < 1e-6


def test_the_same_ray_three_times():
    cfg, geo, vox, row = _row_map()
    view = _view(geo, (2.5, 3.5, 5.5), rng=40 * float(cfg["voxel_size"]))
    one, _, _ = vr.query_views(geo, vox, view, [[1.0, 0.0, 0.0]])
    three, rays, unk = vr.query_views(geo, vox, view, [[1.0, 0.0, 0.0]] * 3)
    for k in ("n_unknown", "n_free", "n_occupied"):
        assert three[k][0] == one[k][0]
    for k in ("rays_hit", "rays_in_map", "ray_cells", "ray_unknown"):
        assert three[k][0] == 3 * one[k][0]
    assert (rays["cells"] == 15).all() and (unk == 5).all()
    # a second ray up the y column of the start cell shares that one cell with the row
    two, _, _ = vr.query_views(geo, vox, view, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    n_y = int(geo.N[1]) - 3
    assert two["n_free"][0] == one["n_free"][0] + n_y - 1 and two["ray_cells"][0] == one["ray_cells"][0] + n_y


def test_view_outside_the_map_looking_in():
    cfg, geo, vox, row = _row_map()
    size = float(cfg["voxel_size"])
    view = _view(geo, (-6.5, 3.5, 5.5), rng=12 * size)      # from 6.5 cells outside to u = 5.5: cells 0..5
    gain, rays, unk = vr.query_views(geo, vox, view, [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    g = gain[0]
    assert (g["n_unknown"], g["n_free"], g["n_occupied"], g["rays_hit"], g["rays_in_map"]) == (0, 6, 0, 0, 1)
    assert list(rays["cells"][0]) == [6, 0] and (rays["voxel"] == qr.INVALID).all() and (rays["t"] == -1).all()
    # turned about y by 90 degrees the camera's z axis points along +x: the same ray from (0, 0, 1)
    turned = _view(geo, (-6.5, 3.5, 5.5), q=(np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0), rng=12 * size)
    g2, r2, _ = vr.query_views(geo, vox, turned, [[0.0, 0.0, 1.0]])
    assert g2["n_free"][0] == 6 and r2["cells"][0, 0] == 6


def test_range_zero_and_non_finite():
    cfg, geo, vox, row = _row_map()
    d = np.array([[1.0, 0.0, 0.0], [0.3, -2.0, 0.1], [np.nan, 0.0, 1.0]], np.float32)
    for rng in (0.0, -3.0):
        gain, rays, unk = vr.query_views(geo, vox, _view(geo, (12.5, 3.5, 5.5), rng=rng), d)   # in an unknown cell
        g = gain[0]
        assert (g["n_unknown"], g["n_free"], g["n_occupied"], g["rays_hit"], g["rays_in_map"], g["ray_cells"], g["ray_unknown"]) == (1, 0, 0, 0, 2, 2, 2)
        assert list(rays["cells"][0]) == [1, 1, 0] and list(unk[0]) == [1, 1, 0]
    gain, rays, unk = vr.query_views(geo, vox, _view(geo, (16.5, 3.5, 5.5), rng=0.0), d[:1])          # in the obstacle: a hit at t = 0
    assert gain["n_occupied"][0] == 1 and gain["rays_hit"][0] == 1 and rays["t"][0, 0] == 0 and rays["voxel"][0, 0] == row[16]
    for field, idx in (("pos", 2), ("q", 0), ("range", None)):
        view = _view(geo, (2.5, 3.5, 5.5), rng=4.0)
        if idx is None:
            view[field] = np.inf
        else:
            view[field][0, idx] = np.nan
        gain, rays, unk = vr.query_views(geo, vox, view, d)
        assert gain.tobytes() == bytes(40) and (rays["cells"] == 0).all() and (rays["t"] == -1).all() and (rays["voxel"] == qr.INVALID).all()
        assert not unk.any()


def test_rays_follow_quat_mat_in_float32():
    rng = np.random.default_rng(7)
    views = np.zeros(5, binding.VIEW)
    views["pos"] = rng.normal(0, 3, (5, 3))
    views["q"] = rng.normal(0, 1, (5, 4))          # used as given: not normalised
    views["range"] = rng.uniform(0.5, 9, 5)
    d = rng.normal(0, 1, (40, 3)).astype(np.float32)
    a, b, given = vr.rays_of(views, d)
    assert given.all() and a.dtype == np.float32 and b.dtype == np.float32
    for v in range(5):
        R = sc.quat_mat(views["q"][v].astype(np.float64))
        assert np.array_equal(vr.rotation(views["q"][v])[0], np.array([[np.float32(x) for x in row] for row in
                                                                        sc.quat_mat(views["q"][v])], np.float32))
        want = views["pos"][v].astype(np.float64) + float(views["range"][v]) * (d.astype(np.float64) @ R.T)
        assert np.abs(b[v] - want).max() < 1e-4 and np.array_equal(a[v], np.broadcast_to(views["pos"][v], (40, 3)))


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_unambiguous_rays_fill_on_every_shape(name):
    cfg = sc.config(name)
    geo = qr.Geometry(cfg, sc.crafted_ring(cfg, sc.crafted_steps(cfg)))
    views = vr.standard_views(geo, 5 + ord(name))
    d = vr.unambiguous_rays(geo, views, 509, 17)
    assert d.shape == (509, 3) and d.dtype == np.float32 and np.isfinite(d).all()
    a, b, given = vr.rays_of(views, d)
    assert given[[0, 1, 2, 3, 4, 5, 7]].all() and not given[6].any()
    for v in (0, 1, 2, 3, 4, 5, 7):
        assert not qr.segment_ambiguous(geo, a[v], b[v]).any()
    on_a_face = views.copy()
    on_a_face["pos"][5] = geo.center + geo.pmin      # the range-0 view on a corner of the map: every one of its rays is ambiguous
    with pytest.raises(ValueError):
        vr.unambiguous_rays(geo, on_a_face, 509, 17)
