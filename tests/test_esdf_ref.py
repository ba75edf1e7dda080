"""The NumPy restatement of the distance field (tests/esdf_ref.py) on the CPU: its min-plus transform against brute
force and against scipy, its query against the definitions (the interpolant hits D at cell centres, the gradient is
the interpolant's derivative)."""
import numpy as np
import pytest

from tests import esdf_ref as er


def _grids():
    rng = np.random.default_rng(7)
    yield rng.random((4, 8, 16)) < 0.05           # non-cubic, sparse
    yield rng.random((8, 4, 8)) < 0.3
    yield np.zeros((4, 4, 8), bool)                # empty
    yield np.ones((4, 8, 4), bool)                 # full
    g = np.zeros((8, 16, 4), bool)
    g[7, 15, 3] = True                             # one obstacle in a corner
    yield g


@pytest.mark.parametrize("k", range(5))
def test_edt_matches_brute_force(k):
    obst = list(_grids())[k]
    d2 = er.edt_d2(obst)
    assert np.array_equal(d2, er.brute_d2(obst))
    if not obst.any():
        assert (d2 == er.INVALID).all()
    if obst.all():
        assert (d2 == 0).all()
    if obst.sum() == 1:
        assert d2[0, 0, 0] == 7 ** 2 + 15 ** 2 + 3 ** 2


def test_edt_matches_scipy():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(8)
    for shape, p in (((16, 32, 64), 0.002), ((32, 16, 32), 0.05), ((8, 64, 16), 0.0005)):
        obst = rng.random(shape) < p
        obst[rng.integers(0, shape[0]), rng.integers(0, shape[1]), rng.integers(0, shape[2])] = True
        ref = nd.distance_transform_edt(~obst, return_distances=False, return_indices=True)
        d2_ref = sum((ref[a] - np.indices(shape)[a]).astype(np.int64) ** 2 for a in range(3))
        assert np.array_equal(er.edt_d2(obst), d2_ref.astype(np.uint32))


def test_check_sites():
    obst = list(_grids())[0]
    d2 = er.edt_d2(obst)
    idx = np.indices(obst.shape)
    # a valid site grid: scipy's, or by brute force here
    z, y, x = np.nonzero(obst)
    gz, gy, gx = idx
    dd = (gx[..., None] - x) ** 2 + (gy[..., None] - y) ** 2 + (gz[..., None] - z) ** 2
    k = dd.argmin(axis=-1)
    site = (x[k] | (y[k] << 4) | (z[k] << 7)).astype(np.uint32)
    nb = (4, 3, 2)
    assert er.check_sites(obst, d2, site, nb) is None
    bad = site.copy()
    z0, y0, x0 = np.argwhere(d2 > 0)[0]
    bad[z0, y0, x0] = x0 | (y0 << 4) | (z0 << 7)     # a cell that is no obstacle as its own site
    assert er.check_sites(obst, d2, bad, nb) is not None
    empty = np.zeros_like(obst)
    assert er.check_sites(empty, er.edt_d2(empty), np.full(obst.shape, er.INVALID, np.uint32), nb) is None


def _field(nb=(4, 3, 3), size=0.3, center=(1.25, -3.5, 0.75)):
    rng = np.random.default_rng(9)
    shape = (1 << nb[2], 1 << nb[1], 1 << nb[0])
    obst = rng.random(shape) < 0.03
    d2 = er.edt_d2(obst)
    z, y, x = np.nonzero(obst)
    gz, gy, gx = np.indices(shape)
    dd = (gx[..., None] - x) ** 2 + (gy[..., None] - y) ** 2 + (gz[..., None] - z) ** 2
    k = dd.argmin(axis=-1)
    site = (x[k] | (y[k] << nb[0]) | (z[k] << (nb[0] + nb[1]))).astype(np.uint32)
    snap = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    geo = er.geometry(nb, size, center)
    return geo, np.float32(size), obst, d2, site, snap


def test_query_interpolant_at_cell_centres_and_rules():
    geo, size, obst, d2, site, snap = _field()
    NZ, NY, NX = obst.shape
    gz, gy, gx = np.indices(obst.shape)
    centres = (geo.center + geo.pmin) + (np.stack([gx, gy, gz], -1).reshape(-1, 3).astype(np.float32) + np.float32(0.5)) * size
    r = er.query_distance(geo, size, d2, site, snap, centres)
    D = np.sqrt(d2.astype(np.float32)) * size
    assert np.allclose(r["distance"], D.reshape(-1).astype(np.float64), rtol=0, atol=1e-6)
    assert np.array_equal(r["d2"], d2.reshape(-1))
    sx, sy, sz = er.site_cells(site.reshape(-1), geo.n_bits)
    assert obst[sz, sy, sx].all()
    w = snap.reshape(-1)[0]
    assert r["track"].dtype == np.uint16 and r["occ"].dtype == np.int8 and w == snap[0, 0, 0]
    assert np.array_equal(r["track"], (snap[sz, sy, sx] & 0xFFFF).astype(np.uint16))
    # no answer: outside, non-finite, and a field without obstacles
    lo, hi = geo.center + geo.pmin, geo.center - geo.pmin
    p = np.array([lo - 0.01, hi, [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    r = er.query_distance(geo, size, d2, site, snap, p)
    assert (r["d2"] == er.INVALID).all() and (r["distance"] == -1).all() and (r["gradient"] == 0).all()
    assert np.isnan(r["nearest"]).all() and (r["occ"] == -1).all() and (r["track"] == 0).all()
    none = np.full_like(site, er.INVALID)
    r = er.query_distance(geo, size, np.full_like(d2, er.INVALID), none, snap, centres[:10])
    assert (r["d2"] == er.INVALID).all() and (r["distance"] == -1).all()
    # the exact lower faces are inside
    r = er.query_distance(geo, size, d2, site, snap, lo[None, :])
    assert r["d2"][0] == d2[0, 0, 0]


def test_query_gradient_is_the_interpolants_derivative():
    geo, size, obst, d2, site, snap = _field()
    rng = np.random.default_rng(10)
    lo, hi = geo.center + geo.pmin, geo.center - geo.pmin
    p = rng.uniform(lo, hi, (3000, 3)).astype(np.float64)
    h = 1e-3 * float(size)
    r = er.query_distance(geo, size, d2, site, snap, p.astype(np.float32))
    u = geo.u(p.astype(np.float32)).astype(np.float64)
    frac = u - 0.5 - np.floor(u - 0.5)
    away = ((frac > 0.05) & (frac < 0.95)).all(axis=1) & (u > 0.6).all(axis=1) & (u < geo.N - 0.6).all(axis=1)
    assert away.sum() > 1000
    for a in range(3):
        dp = np.zeros(3)
        dp[a] = h
        # (positions in float64 only for the difference quotient: the restatement takes u from float32 positions, so
        # step the positions by a float32-representable amount)
        pp, pm = (p + dp).astype(np.float32), (p - dp).astype(np.float32)
        step = (pp[:, a].astype(np.float64) - pm[:, a].astype(np.float64))
        fd = (er.query_distance(geo, size, d2, site, snap, pp)["distance"] - er.query_distance(geo, size, d2, site, snap, pm)["distance"]) / step
        assert np.allclose(r["gradient"][away, a], fd[away], rtol=1e-3, atol=1e-3), a
    # beyond the outermost cell centres the interpolant is constant along that axis
    q = np.tile(lo + np.float32(0.2) * size, (1, 1)).astype(np.float32)
    q[0, 1:] = (geo.center + np.float32(0.3))[1:]
    r = er.query_distance(geo, size, d2, site, snap, q)
    assert r["gradient"][0, 0] == 0
