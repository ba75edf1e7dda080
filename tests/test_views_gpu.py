"""View scoring (sdm_query_views) on the GPU against the NumPy restatement in tests/views_ref.py: every integer field of
every gain, every ray's hit and its unknown-cell count equal with no ray excluded (the ray tables come from
views_ref.unambiguous_rays), and every ray bit for bit what sdm_query_segments returns for the host-built end points.
Crafted random blocks on the map shapes of tests/shape_cases.py (rings shifted on every axis), maps filled by the real
update, one ray and one view, batches forced by sdm_debug_view_batch, device mode in stream order, no side effects on
the map, the argument checks, and the camera frame against the labeled cloud of sdm_update_raw."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import parity_utils as pu
from tests import query_ref as qr
from tests import shape_cases as sc
from tests import views_ref as vr
from tests.test_frontiers_gpu import crafted_map, pattern_block
from tests.test_instances_gpu import DRIVE, MAPS, get_map
from tests.test_queries_gpu import _check_segments

pytestmark = pytest.mark.gpu

N_RAYS = 509     # not a multiple of 64: the last wave of a view is partly idle
REAL = [0, 1, 2, 3, 4, 5, 7]   # of views_ref.standard_views: every view but the one with NaN in pos
_CRAFTED = {}


def crafted(name):
    if name not in _CRAFTED:
        _CRAFTED[name] = crafted_map(name, pattern_block(name, "random"))
    return _CRAFTED[name]


def check_views(g, geo, vox, views, dirs):
    """one host-mode call against the restatement and against sdm_query_segments -> (gain, rays, ray_unknown)"""
    gain, rays, unk = g.query_views(views, dirs, with_rays=True)
    ref_gain, ref_rays, ref_unk = vr.query_views(geo, vox, views, dirs)
    print("n_unknown", gain["n_unknown"], "n_free", gain["n_free"], "n_occupied", gain["n_occupied"], "rays_hit", gain["rays_hit"],
          "ray_unknown", gain["ray_unknown"])
    msg = vr.equal_gain(gain, ref_gain)
    assert msg is None, msg
    assert np.array_equal(unk, ref_unk)
    for k in ("voxel", "cells", "occ", "label", "track"):
        assert np.array_equal(rays[k], ref_rays[k]), k
    a, b, given = vr.rays_of(views, dirs)
    flat = rays.reshape(-1)
    _, ok = _check_segments(geo, vox, flat, a.reshape(-1, 3), b.reshape(-1, 3), False)   # t within its tolerance
    assert np.array_equal(ok, given.reshape(-1))    # no ray excused: only those that visit nothing by definition
    nothing = flat[~given.reshape(-1)]
    assert (nothing["cells"] == 0).all() and (nothing["t"] == -1).all() and (nothing["voxel"] == qr.INVALID).all()
    seg = g.query_segments(a.reshape(-1, 3), b.reshape(-1, 3))
    assert flat.tobytes() == seg.tobytes()
    assert np.array_equal(gain["ray_cells"], rays["cells"].astype(np.int64).sum(axis=1).astype(np.uint64))
    assert np.array_equal(g.query_views(views, dirs).tobytes(), gain.tobytes())   # without the per-ray outputs
    return gain, rays, unk


def standard_case(g, geo, vox, seed):
    views = vr.standard_views(geo, seed)
    dirs = vr.unambiguous_rays(geo, views, N_RAYS, 17)
    gain, rays, unk = check_views(g, geo, vox, views, dirs)
    assert gain[6].tobytes() == bytes(40)                        # NaN in pos
    assert gain["rays_in_map"][5] == N_RAYS and gain["ray_cells"][5] == N_RAYS and gain[5]["n_unknown"] + gain[5]["n_free"] + gain[5]["n_occupied"] == 1
    assert 0 < gain["rays_in_map"][4] < N_RAYS                   # outside looking in: some rays point away
    assert (gain["rays_in_map"][[0, 1, 2, 3, 7]] == N_RAYS).all()
    return views, dirs, gain, rays, unk


# ---- crafted random blocks on every map shape -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_map_shapes(name):
    cfg, g, geo, vox = crafted(name)
    views, dirs, gain, rays, unk = standard_case(g, geo, vox, 5 + ord(name))
    inside = gain[[0, 1, 7]]    # among the block's obstacles and unknown cells (a view may sit in an obstacle: all its rays end there)
    assert inside["n_unknown"].sum() > 0 and (inside["rays_hit"] > 0).all() and (inside["n_occupied"] > 0).all()
    assert (gain["n_occupied"] <= gain["rays_hit"]).all()
    # rays share their cells near the camera: the sum over rays counts them again and again
    assert inside["ray_unknown"].sum() > inside["n_unknown"].sum()
    total = gain["n_unknown"].astype(np.int64) + gain["n_free"] + gain["n_occupied"]
    assert (total <= g.V).all() and (total[REAL] <= gain["ray_cells"][REAL]).all()


# ---- maps filled by the real update -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", MAPS)
def test_real_maps(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    views, dirs, gain, rays, unk = standard_case(g, geo, vox, 23)
    assert gain["n_unknown"].sum() > 0 and gain["n_free"].sum() > 0
    if kind == "dense":
        assert gain["rays_hit"].sum() > 0


# ---- one ray, one view ------------------------------------------------------------------------------------------------
def test_edge_sizes():
    cfg, g, geo, vox = crafted("B")
    views = vr.standard_views(geo, 5 + ord("B"))
    dirs = vr.unambiguous_rays(geo, views, N_RAYS, 17)
    gain, rays, unk = check_views(g, geo, vox, views, dirs[:1])         # n_rays = 1
    assert rays.shape == (8, 1) and (gain["rays_in_map"][REAL] <= 1).all()
    for v in (0, 4, 6):                                                  # n_views = 1
        gain, rays, unk = check_views(g, geo, vox, views[v:v + 1], dirs)
        assert rays.shape == (1, N_RAYS)
    gain, rays, unk = check_views(g, geo, vox, views[7:8], dirs[3:4])    # one of each
    assert rays.shape == (1, 1) and gain["ray_cells"][0] == rays["cells"][0, 0]


# ---- batches: the pool's masks are used again, and must come back empty -----------------------------------------------
def test_batches_and_repeats():
    cfg, g, geo, vox = crafted("C")
    views = np.concatenate([vr.standard_views(geo, s) for s in (31, 32, 31, 33, 34)])   # 40 views, eight of them twice
    dirs = vr.unambiguous_rays(geo, views[:8], N_RAYS, 17)
    want = [x.tobytes() for x in g.query_views(views, dirs, with_rays=True)]
    assert want[0][:8 * 40] == want[0][16 * 40:24 * 40] and want[0][:8 * 40] != want[0][8 * 40:16 * 40]   # a repeated view, the same bytes
    for batch in (3, 1, 40, 7, 0):
        g.set_view_batch(batch)
        for _ in range(2):   # ... and a repeated call
            got = [x.tobytes() for x in g.query_views(views, dirs, with_rays=True)]
            assert got == want, batch
    g.set_view_batch(3)
    ref_gain, _, _ = vr.query_views(geo, vox, views[16:24], dirs)    # batch boundaries inside these eight (the first eight again)
    msg = vr.equal_gain(g.query_views(views, dirs)[16:24], ref_gain)
    g.set_view_batch(0)
    assert msg is None, msg


# ---- device mode, stream order ----------------------------------------------------------------------------------------
def test_device_mode_and_stream_order():
    """A device-mode call after frame k, then frame k + 1, then a second call, one synchronisation: the first answers for
    frame k, the second for frame k + 1 and equals host mode."""
    cfg, params, frames = synth.make_frames("T0", 5, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames[:3]:
        g.update(*f)
    g.synchronize()
    geo_k, vox_k = qr.Geometry(cfg, g.ring_state()), g.voxels()
    views = vr.standard_views(geo_k, 41)
    dirs = vr.unambiguous_rays(geo_k, views, N_RAYS, 17)
    nv, nr = len(views), len(dirs)
    d_views, d_dirs = g.device_put(views), g.device_put(dirs)
    sizes = (nv * 40, nv * nr * 16, nv * nr * 4)
    dtypes = (binding.VIEW_GAIN, binding.SEGMENT_HIT, np.int32)
    o1, o2 = [g.device_alloc(b) for b in sizes], [g.device_alloc(b) for b in sizes]

    def enqueue(o):
        g.query_views(d_views, d_dirs, on_device=True, n_views=nv, n_rays=nr, out=o[0], rays_out=o[1], ray_unknown_out=o[2])

    def fetch(o):
        return [g.device_download(ptr, b).view(dt) for ptr, b, dt in zip(o, sizes, dtypes)]

    enqueue(o1)               # after frame k
    g.update(*frames[3])      # frame k + 1, not waited for
    enqueue(o2)
    g.synchronize()
    r1, r2 = fetch(o1), fetch(o2)
    ref_gain, ref_rays, ref_unk = vr.query_views(geo_k, vox_k, views, dirs)
    msg = vr.equal_gain(r1[0], ref_gain)
    assert msg is None, msg
    assert np.array_equal(r1[2].reshape(nv, nr), ref_unk)
    for k in ("voxel", "cells", "occ", "label", "track"):
        assert np.array_equal(r1[1][k].reshape(nv, nr), ref_rays[k]), k
    host = g.query_views(views, dirs, with_rays=True)
    for x, y in zip(r2, host):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(g.voxels().view(np.uint64), vox_k.view(np.uint64))
    assert r1[0].tobytes() != r2[0].tobytes()
    g.query_views(d_views, d_dirs, on_device=True, n_views=nv, n_rays=nr, out=o1[0])    # without the per-ray outputs
    g.synchronize()
    assert g.device_download(o1[0], sizes[0]).tobytes() == r2[0].tobytes()
    for ptr in [d_views, d_dirs] + o1 + o2:
        g.device_free(ptr)
    g.close()


def test_views_leave_the_map_alone():
    cfg, params, frames = synth.make_frames("T0", 6, n_dynamic=2)
    a = binding.SdmMap(cfg, params, synth.noise_table())
    b = binding.SdmMap(cfg, params, synth.noise_table())
    geo = qr.Geometry(cfg, a.ring_state())
    views = vr.standard_views(geo, 43)
    dirs = np.random.default_rng(6).normal(0, 1, (N_RAYS, 3)).astype(np.float32)
    for f in frames:
        a.update(*f)
        b.update(*f)
        b.query_views(views, dirs, with_rays=True)
        b.query_views(views[:3], dirs[:7])
    a.synchronize()
    b.synchronize()
    rep = pu.compare_maps(a, b, a.S, check_results=True)
    assert not rep, "\n".join(rep)
    assert np.array_equal(a.voxels().view(np.uint64), b.voxels().view(np.uint64))
    assert a.query_views(views, dirs).tobytes() == b.query_views(views, dirs).tobytes()
    a.close()
    b.close()


def test_argument_errors():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, synth.PARAMS["vkitti2"], synth.noise_table())
    L, INV = g.L, 1
    views = np.zeros(4, binding.VIEW)
    views["q"][:, 0] = 1
    dirs = np.ones((4, 3), np.float32)
    out = np.full(4, 0xA5, np.uint8).repeat(40).view(binding.VIEW_GAIN)
    rays = np.zeros(16, binding.SEGMENT_HIT)
    unk = np.zeros(16, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.sdm_query_views(None, vp(views), 4, vp(dirs), 4, vp(out), None, None, 0) == INV
    assert L.sdm_query_views(g.h, None, 4, vp(dirs), 4, vp(out), None, None, 0) == INV
    assert L.sdm_query_views(g.h, vp(views), 4, None, 4, vp(out), None, None, 0) == INV
    assert L.sdm_query_views(g.h, vp(views), 4, vp(dirs), 4, None, None, None, 0) == INV
    assert L.sdm_query_views(g.h, vp(views), -1, vp(dirs), 4, vp(out), None, None, 0) == INV
    assert L.sdm_query_views(g.h, vp(views), 4, vp(dirs), 0, vp(out), None, None, 0) == INV
    assert L.sdm_query_views(g.h, vp(views), 4, vp(dirs), -3, vp(out), None, None, 0) == INV
    assert L.sdm_query_views(g.h, vp(views), 4, vp(dirs), 65537, vp(out), None, None, 0) == INV
    assert "n_rays" in L.sdm_last_error().decode()
    assert L.sdm_query_views(g.h, vp(views), 1 << 15, vp(dirs), 65536, vp(out), None, None, 0) == INV      # 2^31 rays
    assert L.sdm_query_views(g.h, vp(views), 1 << 60, vp(dirs), 4, vp(out), None, None, 0) == INV
    assert L.sdm_query_views(g.h, vp(views), 4, vp(dirs), 4, vp(out), None, None, 0x2) == INV              # unknown blocks: not for views
    assert L.sdm_query_views(g.h, vp(views), 4, vp(dirs), 4, vp(out), None, None, 0x80000000) == INV
    assert (out.view(np.uint8) == 0xA5).all()    # nothing written by a refused call
    for fl in (0, 1):
        assert L.sdm_query_views(g.h, vp(views), 0, vp(dirs), 4, vp(out), None, None, fl) == 0
    assert (out.view(np.uint8) == 0xA5).all()
    assert L.sdm_query_views(g.h, vp(views), 4, vp(dirs), 4, vp(out), vp(rays), vp(unk), 0) == 0
    assert (out["pad"] == 0).all() and (out["rays_in_map"] == 4).all() and (unk >= 0).all()
    assert L.sdm_debug_view_batch(None, 1) == INV and L.sdm_debug_view_batch(g.h, -5) == 0
    g.close()
    s = binding.SdmMap(cfg, synth.PARAMS["vkitti2"], synth.noise_table(), shard_rank=0, shard_count=2)
    assert s.L.sdm_query_views(s.h, vp(views), 4, vp(dirs), 4, vp(out), None, None, 0) == INV
    assert "shard" in s.L.sdm_last_error().decode()
    with pytest.raises(binding.SdmError):
        s.query_views(views, dirs)
    s.close()


# ---- the camera frame: a view's rays are the rays of the camera sdm_update_raw back-projects through ------------------
def test_camera_frame_matches_the_labeled_cloud():
    from tests.test_labeled_cloud import frame_and_raw
    cfg, params, scene, depth, cloud, static_mask, objects, pos64, q64 = frame_and_raw("T0", "vkitti2", 2, n_dynamic=2)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    g.update_raw(depth, static_mask, synth.LABEL_TO_STATIC_INSTANCE, objects, pos64, q64, sync=True)
    got = g.labeled_cloud()
    geo = qr.Geometry(cfg, g.ring_state())
    table = binding.pinhole_rays(g.cfg, 1)
    assert table.shape == (cfg["height"], cfg["width"], 3)
    # one view per depth value would be one call per pixel: the restatement's ray formula with range = the pixel's depth
    view = np.zeros(1, binding.VIEW)
    view["pos"], view["q"], view["range"] = pos64.astype(np.float32), q64.astype(np.float32), 1.0
    z = np.asarray(depth, np.float32).reshape(-1)
    valid = (got["is_valid"] != 0) & np.isfinite(z)
    assert valid.sum() > 1000
    a, b1, given = vr.rays_of(view, table.reshape(-1, 3))            # range 1: b1 - pos = R d, bit for bit (1 * x = x)
    R = vr.rotation(view["q"])[0]
    d = table.reshape(-1, 3)
    rd = np.stack([(R[i, 0] * d[:, 0] + R[i, 1] * d[:, 1]) + R[i, 2] * d[:, 2] for i in range(3)], axis=1)
    with np.errstate(invalid="ignore"):
        end = view["pos"][0][None, :] + z[:, None] * rd
    assert end.dtype == np.float32
    p = np.stack([got["x"], got["y"], got["z"]], axis=1)
    u_end, u_p = geo.u(end[valid]).astype(np.float64), geo.u(p[valid]).astype(np.float64)
    clear = (np.abs(u_p - np.round(u_p)) > qr.AMBIGUOUS_VOXELS).all(axis=1)
    # (how many pixels are clear is the scene's affair - its walls and boxes lie on round coordinates, so whole surfaces sit
    # on cell faces -; the check only needs a population to hold for: as many clear pixels as valid ones were asked for above)
    print("valid pixels", int(valid.sum()), "of them farther than", qr.AMBIGUOUS_VOXELS, "voxel from a cell face:", int(clear.sum()))
    assert clear.sum() > 1000
    assert np.array_equal(np.floor(u_end[clear]), np.floor(u_p[clear]))
    # ... and the library's rays are those: a view of range z0 ends its ray of pixel (v, u) in the cell of that pixel's point
    i = int(np.flatnonzero(valid)[np.flatnonzero(clear)[0]])
    view["range"] = z[i]
    a, b, _ = vr.rays_of(view, d[i:i + 1])
    assert np.array_equal(b[0, 0], end[i])
    hit = g.query_views(view, d[i:i + 1], with_rays=True)[1][0, 0]
    assert hit.tobytes() == g.query_segments(a[0], b[0])[0].tobytes()
    g.close()
