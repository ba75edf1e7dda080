"""The batched map queries (sdm_query_points / _segments / _boxes) on the GPU against the NumPy restatement in
tests/query_ref.py, on maps whose result arrays were filled by the real update: a random dense state with stale slabs
followed by a short synthetic drive, and the drive alone (its ring shifts on two axes under way).  Also device mode
(device buffers in HBM, stream order across frames), no side effects on the map, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import parity_utils as pu
from tests import query_ref as qr
from tests.dense_state import random_state, stamps_for

pytestmark = pytest.mark.gpu

# a short drive that moves sideways as well as forwards: the ring shifts on x and z under way
DRIVE = dict(n_dynamic=2, lateral_extra=(0, 0.5))
_MAPS, _FRAMES = {}, {}


def _frames(name):
    if name not in _FRAMES:
        _FRAMES[name] = synth.make_frames(name, 6, **DRIVE)
    return _FRAMES[name]


def _dense_map(name):
    """a random dense state (stale slabs behind re-stamped slabs), then the drive"""
    cfg, params, frames = _frames(name)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    st = random_state(cfg, 41)
    (sx, sy, sz), ring = stamps_for(g)
    g.load_state(st)
    g.set_stamps(sx, sy, sz)
    g.set_ring_state(ring)
    for f in frames:
        g.update(*f)
    g.synchronize()
    return cfg, g


def _driven_map(name):
    cfg, params, frames = _frames(name)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames:
        g.update(*f)
    g.synchronize()
    return cfg, g


def get_map(kind, name):
    key = (kind, name)
    if key not in _MAPS:
        _MAPS[key] = (_dense_map if kind == "dense" else _driven_map)(name)
    cfg, g = _MAPS[key]
    ring = g.ring_state()
    assert sum(e != 0 for e in ring["eq_steps"]) >= 2
    return cfg, g, qr.Geometry(cfg, ring), g.voxels()


MAPS = [("dense", "T0"), ("dense", "C1"), ("driven", "T0"), ("driven", "C1")]


def _span(geo, margin_voxels):
    size = np.float32(1) / geo.recip
    return geo.center + geo.pmin - margin_voxels * size, geo.center - geo.pmin + margin_voxels * size


@pytest.mark.parametrize("kind,name", MAPS)
def test_points(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    rng = np.random.default_rng(1)
    lo, hi = _span(geo, 2)
    p = rng.uniform(lo, hi, (200000, 3)).astype(np.float32)
    size = np.float32(1) / geo.recip
    p[:1000] = rng.uniform(lo + 2 * size, hi - 2 * size, (1000, 3)).astype(np.float32)
    p[:1000, 1] = (geo.center + geo.pmin)[1] - rng.random(1000).astype(np.float32) * size   # the (-1, 0) sliver below a face
    p[1000:1100] = geo.center + geo.pmin                                                  # exact faces
    p[1100:1200] = geo.center - geo.pmin
    p[1200:1210, 0] = np.nan
    p[1210:1220, 2] = np.inf
    p[1220:1230, 1] = -np.inf
    res, idx = g.query_points(p, with_index=True)
    ref, ref_idx = qr.query_points(geo, vox, p)
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(res.view(np.uint64), ref.view(np.uint64))
    assert (idx[1200:1230] == qr.INVALID).all() and (res["occ"][1200:1230] == -1).all()
    assert (res["occ"] >= 1).any() and (idx[:1000] != qr.INVALID).any()
    assert np.array_equal(g.query_points(p[:1000]).view(np.uint64), res[:1000].view(np.uint64))


def _hand_segments(geo):
    """(a, b) rows: along x across the ring's wrap point, entirely outside, entering from outside, zero length, 1 km"""
    size = np.float32(1) / geo.recip
    c0 = geo.center + geo.pmin
    wrap_x = (geo.N[0] - geo.eq[0]) % geo.N[0]   # map x index whose ring index is 0
    y, z = c0[1] + 3.37 * size, c0[2] + 5.61 * size
    rows = [
        ([c0[0] + (wrap_x - 3.3) * size, y, z], [c0[0] + (wrap_x + 3.4) * size, y, z]),
        ([c0[0] + 0.2 * size, y, z], [c0[0] + (geo.N[0] - 0.3) * size, y, z]),
        ([c0[0] - 5.3 * size, y, z], [c0[0] - 1.7 * size, y + 2.1 * size, z]),           # entirely outside
        ([c0[0] - 4.3 * size, y, z], [c0[0] + 6.7 * size, y + 1.3 * size, z + 0.7 * size]),  # enters
        ([c0[0] + 7.3 * size, y, z], [c0[0] + 7.3 * size, y, z]),                        # zero length
        ([c0[0] - 500.0, y, z - 0.1], [c0[0] + 500.0, y + 0.3, z + 0.2]),               # 1 km
    ]
    a = np.array([r[0] for r in rows], np.float32)
    b = np.array([r[1] for r in rows], np.float32)
    return a, b


def _check_segments(geo, vox, got, a, b, unknown_blocks):
    ref = qr.query_segments(geo, vox, a, b, unknown_blocks=unknown_blocks)
    ok = ~qr.segment_ambiguous(geo, a, b)
    for k in ("voxel", "cells", "occ", "label", "track"):
        bad = np.flatnonzero(ok & (got[k] != ref[k]))
        assert not len(bad), (k, unknown_blocks, bad[:5], got[bad[:3]], {kk: ref[kk][bad[:3]] for kk in ref})
    L = np.linalg.norm(geo.u(b).astype(np.float64) - geo.u(a).astype(np.float64), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = 1e-5 + np.where(L > 0, 2e-3 / L, 0)
    dt = np.abs(got["t"].astype(np.float64) - ref["t"])
    assert not (ok & (dt > tol)).any()
    return ref, ok


@pytest.mark.parametrize("kind,name", MAPS)
def test_segments(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    rng = np.random.default_rng(2)
    lo, hi = _span(geo, 2)
    n = 50000
    a = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    b = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    short = rng.random(n) < 0.3
    b[short] = a[short] + rng.normal(0, 3 / geo.recip, (short.sum(), 3)).astype(np.float32)
    a[10:20, 1] = np.nan
    b[20:30, 2] = np.inf
    for ub in (False, True):
        got = g.query_segments(a, b, unknown_blocks=ub)
        ref, ok = _check_segments(geo, vox, got, a, b, ub)
        assert ok.mean() > 0.5
        assert (got["voxel"][ok] != qr.INVALID).any()
        if not ub:
            assert (got["t"][ok] < 0).any()
        assert (got["cells"][10:30] == 0).all() and (got["t"][10:30] == (0.0 if ub else -1.0)).all()
    ha, hb = _hand_segments(geo)
    limit = int(geo.N.sum())
    for ub in (False, True):
        got = g.query_segments(ha, hb, unknown_blocks=ub)
        ref, ok = _check_segments(geo, vox, got, ha, hb, ub)
        assert ok.all()
        assert got["cells"][2] == 0 and (got["t"][2] == (0.0 if ub else -1.0))
        assert (got["cells"] <= limit).all()
    # the walk itself, with nothing blocking: a full x row through the wrap point, the 1 km segment clipped to the map
    empty = np.zeros_like(vox)
    _, walks = qr.query_segments(geo, empty, ha, hb, record=True)
    assert len(walks[1]) == geo.N[0] and len(walks[4]) == 1 and len(walks[2]) == 0
    assert len(walks[5]) <= limit and len(walks[5]) >= geo.N[0]


@pytest.mark.parametrize("kind,name", MAPS)
def test_boxes(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    rng = np.random.default_rng(3)
    lo, hi = _span(geo, 3)
    n = 20000
    size = np.float32(1) / geo.recip
    blo = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    bhi = (blo + rng.random((n, 3)).astype(np.float32) * 8 * size).astype(np.float32)
    blo[0], bhi[0] = geo.center + geo.pmin, geo.center - geo.pmin - np.float32(1e-3) * size   # the whole map
    blo[1], bhi[1] = lo, hi                                                                    # sticking out everywhere
    blo[2:200], bhi[2:200] = bhi[2:200], blo[2:200] - size                                     # inverted
    blo[200:210, 0] = np.nan
    got = g.query_boxes(blo, bhi)
    ref = qr.query_boxes(geo, vox, blo, bhi)
    for k in ref:
        bad = np.flatnonzero(got[k] != ref[k])
        assert not len(bad), (k, bad[:5], got[bad[:3]], ref[k][bad[:3]])
    V = len(vox)
    assert got["n_occupied"][0] + got["n_free"][0] + got["n_unknown"][0] == V and got["clipped"][0] == 0
    assert got["n_occupied"][1] + got["n_free"][1] + got["n_unknown"][1] == V and got["clipped"][1] == 1
    assert got["clipped"][2:210].sum() == 0 and got["n_free"][2:210].sum() == 0
    assert (got["clipped"] == 1).sum() > 1000 and (got["first_occupied"] != qr.INVALID).sum() > 100


def test_device_mode_and_stream_order():
    """Device pointers in HBM (the library's own buffers: INTEGRATION.md - no second HIP runtime in the process), results
    equal to host mode; a query enqueued after frame k, then frame k+1, then a second query, one synchronisation: the
    first answers for frame k, the second for frame k+1."""
    cfg, params, frames = synth.make_frames("T0", 5, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames[:3]:
        g.update(*f)
    g.synchronize()
    rng = np.random.default_rng(4)
    geo_k, vox_k = qr.Geometry(cfg, g.ring_state()), g.voxels()
    lo, hi = _span(geo_k, 1)
    n = 30000
    p = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    ab = np.ascontiguousarray(np.concatenate([p, rng.uniform(lo, hi, (n, 3)).astype(np.float32)], axis=1))
    bx = np.ascontiguousarray(np.concatenate([p, p + np.float32(1.5)], axis=1))
    ins = [g.device_put(x) for x in (p, ab, bx)]
    sizes = (n * 8, n * 4, n * 16, n * 20)
    dtypes = (binding.VOXEL_RESULT, np.uint32, binding.SEGMENT_HIT, binding.BOX_RESULT)
    o1, o2 = [g.device_alloc(b) for b in sizes], [g.device_alloc(b) for b in sizes]

    def enqueue(o):
        g.query_points(ins[0], on_device=True, n=n, out=o[0], voxel_out=o[1])
        g.query_segments(ins[1], on_device=True, n=n, out=o[2], unknown_blocks=True)
        g.query_boxes(ins[2], on_device=True, n=n, out=o[3])

    def fetch(o):
        return [g.device_download(ptr, b).view(dt) for ptr, b, dt in zip(o, sizes, dtypes)]

    enqueue(o1)               # after frame k
    g.update(*frames[3])      # frame k+1, not waited for
    enqueue(o2)
    g.synchronize()
    r1, r2 = fetch(o1), fetch(o2)
    # the first query answered for frame k
    ref_p, ref_i = qr.query_points(geo_k, vox_k, p)
    assert np.array_equal(r1[0].view(np.uint64), ref_p.view(np.uint64)) and np.array_equal(r1[1], ref_i)
    seg_k = qr.query_segments(geo_k, vox_k, ab[:, :3], ab[:, 3:], unknown_blocks=True)
    ok = ~qr.segment_ambiguous(geo_k, ab[:, :3], ab[:, 3:])
    assert np.array_equal(r1[2]["voxel"][ok], seg_k["voxel"][ok]) and np.array_equal(r1[2]["cells"][ok], seg_k["cells"][ok])
    box_k = qr.query_boxes(geo_k, vox_k, bx[:, :3], bx[:, 3:])
    assert all(np.array_equal(r1[3][k], box_k[k]) for k in box_k)
    # the second one for frame k+1, and equal to host mode
    h = (*g.query_points(p, with_index=True), g.query_segments(ab[:, :3], ab[:, 3:], unknown_blocks=True),
         g.query_boxes(bx[:, :3], bx[:, 3:]))
    for x, y in zip(r2, h):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert not np.array_equal(g.voxels().view(np.uint64), vox_k.view(np.uint64))
    assert not np.array_equal(r1[0].view(np.uint64), r2[0].view(np.uint64))
    for ptr in ins + o1 + o2:
        g.device_free(ptr)
    g.close()


def test_queries_leave_the_map_alone():
    cfg, params, frames = synth.make_frames("T0", 6, n_dynamic=2)
    a = binding.SdmMap(cfg, params, synth.noise_table())
    b = binding.SdmMap(cfg, params, synth.noise_table())
    rng = np.random.default_rng(5)
    geo = qr.Geometry(cfg, a.ring_state())
    lo, hi = _span(geo, 2)
    p = rng.uniform(lo - 3, hi + 3, (5000, 3)).astype(np.float32)
    q = rng.uniform(lo - 3, hi + 3, (5000, 3)).astype(np.float32)
    for f in frames:
        a.update(*f)
        b.update(*f)
        b.query_points(p, with_index=True)
        b.query_segments(p, q)
        b.query_segments(p, q, unknown_blocks=True)
        b.query_boxes(np.minimum(p, q), np.maximum(p, q))
    a.synchronize()
    b.synchronize()
    rep = pu.compare_maps(a, b, a.S, check_results=True)
    assert not rep, "\n".join(rep)
    assert np.array_equal(a.voxels().view(np.uint64), b.voxels().view(np.uint64))
    a.close()
    b.close()


def test_argument_errors():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, synth.PARAMS["vkitti2"], synth.noise_table())
    L = g.L
    p = np.zeros((4, 6), np.float32)
    o = np.zeros(64, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    INV = 1
    assert L.sdm_query_points(None, vp(p), 1, vp(o), None, 0) == INV
    assert L.sdm_query_points(g.h, None, 1, vp(o), None, 0) == INV
    assert L.sdm_query_points(g.h, vp(p), 1, None, None, 0) == INV
    assert L.sdm_query_points(g.h, vp(p), -1, vp(o), None, 0) == INV
    assert L.sdm_query_points(g.h, vp(p), 1, vp(o), None, 0x2) == INV
    assert L.sdm_query_segments(g.h, vp(p), 1, vp(o), 0x4) == INV
    assert L.sdm_query_segments(g.h, None, 1, vp(o), 0) == INV
    assert L.sdm_query_boxes(g.h, vp(p), 1, None, 0) == INV
    assert L.sdm_query_boxes(g.h, vp(p), 1, vp(o), 0x8) == INV
    for fl in (0, 1):
        assert L.sdm_query_points(g.h, vp(p), 0, vp(o), None, fl) == 0
        assert L.sdm_query_segments(g.h, vp(p), 0, vp(o), fl) == 0
        assert L.sdm_query_boxes(g.h, vp(p), 0, vp(o), fl) == 0
    assert L.sdm_query_segments(g.h, vp(p), 4, vp(o), 0x3 & ~0x1) == 0   # host mode, unknown blocks: a valid call
    g.close()
    s = binding.SdmMap(cfg, synth.PARAMS["vkitti2"], synth.noise_table(), shard_rank=0, shard_count=2)
    assert s.L.sdm_query_points(s.h, vp(p), 1, vp(o), None, 0) == INV
    assert "shard" in s.L.sdm_last_error().decode()
    assert s.L.sdm_query_segments(s.h, vp(p), 1, vp(o), 0) == INV
    assert s.L.sdm_query_boxes(s.h, vp(p), 1, vp(o), 0) == INV
    with pytest.raises(binding.SdmError):
        s.query_boxes(p[:, :3], p[:, 3:])
    s.close()
