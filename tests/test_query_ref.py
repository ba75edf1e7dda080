"""CPU checks of tests/query_ref.py, the NumPy restatement the GPU tests of the batched map queries compare against:
its cell walk against dense sampling of the segment, its box enumeration against a brute-force meshgrid, and its point
mapping against the CPU oracle's own position -> voxel function on shifted rings."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import query_ref as qr

RING = {"global_time_stamp": 3, "moved_steps": [5, -3, 9], "eq_steps": [5, 29, 9], "map_center": [1.0, -0.6, 1.8],
        "last_pos": [1.0, -0.6, 1.8], "birth_cursor": 0, "move_cursor": 0}


def _geo(name="T0", ring=RING):
    cfg = synth.CONFIGS[name]
    return cfg, qr.Geometry(cfg, ring)


def _random_segments(geo, rng, n, margin=2.0):
    lo = geo.center + geo.pmin - margin / geo.recip
    hi = geo.center - geo.pmin + margin / geo.recip
    a = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    b = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    return a, b


def _sampled_walk(geo, a, b):
    """in-map cells floor(u(t)) along the segment, t sampled every 4e-4 voxel, consecutive repeats merged"""
    ua, ub = geo.u(a)[0].astype(np.float64), geo.u(b)[0].astype(np.float64)
    L = float(np.linalg.norm(ub - ua))
    t = np.linspace(0.0, 1.0, max(int(L / 4e-4) + 2, 2))
    c = np.floor(ua[None, :] + t[:, None] * (ub - ua)[None, :]).astype(np.int64)
    c = c[((c >= 0) & (c < geo.N)).all(axis=1)]
    if len(c) == 0:
        return []
    keep = np.ones(len(c), bool)
    keep[1:] = (c[1:] != c[:-1]).any(axis=1)
    return [tuple(int(v) for v in x) for x in c[keep]]


def test_walk_matches_dense_sampling():
    cfg, geo = _geo()
    rng = np.random.default_rng(3)
    a, b = _random_segments(geo, rng, 3000)
    # a few short ones, and axis-parallel ones
    a[:200], b[:200] = a[:200], a[:200] + rng.normal(0, 0.5, (200, 3)).astype(np.float32)
    b[200:300, 1:] = a[200:300, 1:]
    amb = qr.segment_ambiguous(geo, a, b)
    ok = np.flatnonzero(~amb)[:2000]
    assert len(ok) == 2000
    _, walks = qr.query_segments(geo, None, a[ok], b[ok], record=True)
    n_cells = 0
    for j, i in enumerate(ok):
        ref = _sampled_walk(geo, a[i:i + 1], b[i:i + 1])
        assert walks[j] == ref, (i, a[i], b[i], walks[j][:8], ref[:8])
        n_cells += len(ref)
    assert n_cells > 20000  # (the segments do cross the map)


def test_walk_clips_to_the_map():
    cfg, geo = _geo()
    far = np.float32(1000.0)
    a = np.array([[-far, 0.1, 0.3]], np.float32) + geo.center
    b = np.array([[far, 0.1, 0.3]], np.float32) + geo.center
    out, walks = qr.query_segments(geo, None, a, b, record=True)
    assert len(walks[0]) == geo.N[0] and [c[0] for c in walks[0]] == list(range(geo.N[0]))
    assert out["cells"][0] == geo.N[0]


def test_box_enumeration_matches_meshgrid():
    cfg, geo = _geo()
    rng = np.random.default_rng(5)
    V = int(np.prod(geo.N))
    vox = np.zeros(V, binding.VOXEL_RESULT)
    vox["occ"] = rng.choice([-1, 0, 1, 2], V)
    lo0 = geo.center + geo.pmin - 1.0
    span = -2 * geo.pmin + 2.0
    n = 300
    lo = (lo0 + rng.random((n, 3)) * span).astype(np.float32)
    hi = (lo + rng.random((n, 3)) * span * 0.3).astype(np.float32)
    out = qr.query_boxes(geo, vox, lo, hi)
    vgrid = geo.voxel_grid()
    for i in range(n):
        cells = qr.box_cells_meshgrid(geo, lo[i:i + 1], hi[i:i + 1])
        v = vgrid[cells[:, 2], cells[:, 1], cells[:, 0]]
        o = vox["occ"][v]
        assert out["n_occupied"][i] == (o >= 1).sum() and out["n_free"][i] == (o == 0).sum() and out["n_unknown"][i] == (o == -1).sum()
        assert out["first_occupied"][i] == (v[o >= 1].min() if (o >= 1).any() else qr.INVALID)
        u0, u1 = np.floor(geo.u(lo[i])[0]), np.floor(geo.u(hi[i])[0])
        assert out["clipped"][i] == int((u0 < 0).any() or (u1 >= geo.N).any())
    inv = qr.query_boxes(geo, vox, hi[:5], lo[:5] - 1.0)
    assert not inv["n_occupied"].any() and not inv["n_free"].any() and not inv["n_unknown"].any() and not inv["clipped"].any()


@pytest.mark.parametrize("name", ["T0", "T1"])
def test_point_mapping_matches_the_oracle(name):
    from oracle import oracle as orc
    cfg, geo = _geo(name, dict(RING, eq_steps=[7, 3, 11]))
    o = orc.OracleMap(dict(cfg, bin_order=1), synth.PARAMS["vkitti2"])
    o.set_ring_state(dict(RING, eq_steps=[7, 3, 11]))
    assert o.ring_state()["eq_steps"] == [7, 3, 11]
    rng = np.random.default_rng(11)
    lo = geo.center + geo.pmin
    hi = geo.center - geo.pmin
    size = 1.0 / float(geo.recip)
    p = rng.uniform(lo - 2 * size, hi + 2 * size, (6000, 3)).astype(np.float32)
    p[:500, 0] = lo[0] - rng.random(500).astype(np.float32) * np.float32(size)   # the (-1, 0) sliver below the x face
    p[500:600] = lo                                                             # exact faces
    p[600:700] = hi
    vox = np.zeros(int(np.prod(geo.N)), binding.VOXEL_RESULT)
    _, idx = qr.query_points(geo, vox, p)
    ref = np.array([o.pos_to_voxel(float(x), float(y), float(z)) for x, y, z in p], np.uint64).astype(np.uint32)
    assert np.array_equal(idx, ref)
    assert (idx != qr.INVALID).sum() > 3000 and (idx[:500] != qr.INVALID).any()
