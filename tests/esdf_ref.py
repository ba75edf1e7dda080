"""NumPy restatement of the distance field and the distance query (include/sdm.h: sdm_esdf_update / sdm_get_esdf /
sdm_query_distance), for the tests.

Grids are indexed [z, y, x] in map-index order (the order the field is stored in).  From what a caller can read back -
voxels(), ring_state(), the configuration - it gives:
  * the obstacle grid of a snapshot under the flags, and the snapshot word (track | label << 16 | occ << 24) of every cell;
  * the exact squared distance d2 in cells, as a min-plus transform along each axis in int64, chunked (and by brute
    force over every obstacle, for small grids);
  * the distance query: the point's cell, d2, nearest, track / label / occ from a given site grid (the field may pick
    any of several equally near obstacles, so the site grid is checked on its own: check_sites), the no-answer rule,
    all in float32 as specified; the trilinear interpolant of D and its gradient in float64 over float32 inputs.
"""
import numpy as np

from tests import query_ref as qr

INVALID = 0xFFFFFFFF
UNKNOWN_IS_OBSTACLE = 0x1
STATIC_ONLY = 0x2
_INF = np.int64(1) << 40


def snapshot_grid(geo, voxels):
    """the second word of every cell's result (track, label, occ), [z, y, x]"""
    return voxels.view(np.uint32).reshape(-1, 2)[:, 1][geo.voxel_grid()]


def obstacle_grid(geo, voxels, max_movable, flags=0):
    occ = voxels["occ"][geo.voxel_grid()].astype(np.int32)
    track = voxels["track"][geo.voxel_grid()].astype(np.int32)
    obst = occ >= 1
    if flags & UNKNOWN_IS_OBSTACLE:
        obst |= occ == -1
    if flags & STATIC_ONLY:
        obst &= ~((track >= 1) & (track <= max_movable))
    return obst


def _min_plus_last_axis(g, periodic=False, chunk_bytes=1 << 26):
    """out[..., i] = min_j g[..., j] + (i - j)^2, g int64 (>= _INF = none); periodic: |i - j| taken around a ring"""
    N = g.shape[-1]
    flat = g.reshape(-1, N)
    out = np.empty_like(flat)
    idx = np.arange(N, dtype=np.int64)
    dist = np.abs(idx[:, None] - idx[None, :])
    sq = (np.minimum(dist, N - dist) if periodic else dist) ** 2          # [i, j]
    rows = max(1, chunk_bytes // (8 * N * N))
    for r0 in range(0, len(flat), rows):
        blk = flat[r0:r0 + rows]
        out[r0:r0 + rows] = (blk[:, None, :] + sq[None, :, :]).min(axis=2)
    return np.minimum(out, _INF).reshape(g.shape)


def edt_d2(obst, periodic=()):
    """exact squared Euclidean distance (cells) of every cell to the nearest True of obst [z, y, x] -> uint32, 0xffffffff
    everywhere if there is none.  periodic: map axes (0 = x, 1 = y, 2 = z) measured as a torus - the field a
    computation across the ring's wrap point would give, for the tests to show that theirs differs"""
    g = np.where(obst, np.int64(0), _INF)
    for ax in (2, 1, 0):                              # x, y, z
        g = np.moveaxis(_min_plus_last_axis(np.moveaxis(g, ax, -1), periodic=(2 - ax) in periodic), -1, ax)
    return np.where(g >= _INF, np.int64(INVALID), g).astype(np.uint32)


def brute_d2(obst):
    z, y, x = np.nonzero(obst)
    out = np.full(obst.shape, INVALID, np.uint32)
    if not len(x):
        return out
    gz, gy, gx = np.meshgrid(*(np.arange(n) for n in obst.shape), indexing="ij")
    best = np.full(obst.shape, _INF, np.int64)
    for sx, sy, sz in zip(x, y, z):
        best = np.minimum(best, (gx - sx) ** 2 + (gy - sy) ** 2 + (gz - sz) ** 2)
    return best.astype(np.uint32)


def site_cells(site, n_bits):
    """site word -> (x, y, z) int64 arrays"""
    s = np.asarray(site, np.int64)
    xn, yn = int(n_bits[0]), int(n_bits[1])
    return s & ((1 << xn) - 1), (s >> xn) & ((1 << yn) - 1), s >> (xn + yn)


def check_sites(obst, d2, site, n_bits):
    """the field's site grid is valid: every site an obstacle at exactly the squared distance d2 (None, or a message)"""
    none = d2 == INVALID
    if not np.array_equal(site == INVALID, none):
        return "site / d2 sentinels disagree at %d cells" % int(((site == INVALID) != none).sum())
    if none.all():
        return None
    sx, sy, sz = site_cells(site[~none], n_bits)
    NZ, NY, NX = obst.shape
    if (sx >= NX).any() or (sy >= NY).any() or (sz >= NZ).any():
        return "site outside the map"
    if not obst[sz, sy, sx].all():
        return "%d sites are not obstacles" % int((~obst[sz, sy, sx]).sum())
    gz, gy, gx = np.nonzero(~none)
    got = (gx - sx) ** 2 + (gy - sy) ** 2 + (gz - sz) ** 2
    bad = got != d2[~none].astype(np.int64)
    if bad.any():
        return "%d sites are not at distance d2" % int(bad.sum())
    return None


def query_distance(geo, voxel_size, d2, site, snap, xyz):
    """-> DISTANCE_RESULT-like dict of arrays (gradient, nearest: (n, 3)) for the field (d2, site, snap [z, y, x]) whose
    snapshot geometry is geo; distance and gradient in float64 (the kernel blends in float32)"""
    size = np.float32(voxel_size)
    u = geo.u(xyz)
    n = len(u)
    Nf = geo.N.astype(np.float32)
    with np.errstate(invalid="ignore"):
        ok = ((u >= 0) & (u < Nf)).all(axis=1)
    cell = np.where(ok[:, None], np.floor(np.where(ok[:, None], u, 0)), 0).astype(np.int64)
    sc = np.full(n, INVALID, np.uint32)
    sc[ok] = site[cell[ok, 2], cell[ok, 1], cell[ok, 0]]
    ok &= sc != INVALID
    out = dict(distance=np.full(n, -1.0), gradient=np.zeros((n, 3)), nearest=np.full((n, 3), np.nan, np.float32),
               d2=np.full(n, INVALID, np.uint32), track=np.zeros(n, np.uint16), label=np.zeros(n, np.uint8),
               occ=np.full(n, -1, np.int8), dmax=np.zeros(n))
    if not ok.any():
        return out
    uu = u[ok]
    s = (uu - np.float32(0.5)).astype(np.float32)
    i0 = np.floor(s)
    t = (s - i0).astype(np.float32).astype(np.float64)
    i0 = i0.astype(np.int64)
    c0 = np.clip(i0, 0, geo.N - 1)
    c1 = np.clip(i0 + 1, 0, geo.N - 1)
    D = {}
    for bx in (0, 1):
        for by in (0, 1):
            for bz in (0, 1):
                cx, cy, cz = (c1 if bx else c0)[:, 0], (c1 if by else c0)[:, 1], (c1 if bz else c0)[:, 2]
                D[bx, by, bz] = (np.sqrt(d2[cz, cy, cx].astype(np.float32)) * size).astype(np.float32).astype(np.float64)
    w = [(1 - t[:, a], t[:, a]) for a in range(3)]
    val = np.zeros(len(uu))
    grad = np.zeros((len(uu), 3))
    for (bx, by, bz), Dk in D.items():
        b = (bx, by, bz)
        val += w[0][bx] * w[1][by] * w[2][bz] * Dk
        for a in range(3):
            others = [w[o][b[o]] for o in range(3) if o != a]
            grad[:, a] += (1.0 if b[a] else -1.0) * others[0] * others[1] * Dk
    recip = np.float64(geo.recip)
    out["distance"][ok] = val
    out["gradient"][ok] = grad * recip
    out["dmax"][ok] = np.max(np.stack(list(D.values()), axis=1), axis=1)
    sx, sy, sz = site_cells(sc[ok], geo.n_bits)
    sites = np.stack([sx, sy, sz], axis=1).astype(np.float32)
    out["nearest"][ok] = (geo.center + geo.pmin) + (sites + np.float32(0.5)) * size
    c = cell[ok]
    out["d2"][ok] = ((c[:, 0] - sx) ** 2 + (c[:, 1] - sy) ** 2 + (c[:, 2] - sz) ** 2).astype(np.uint32)
    w1 = snap[sz, sy, sx]
    out["track"][ok] = (w1 & 0xFFFF).astype(np.uint16)
    out["label"][ok] = ((w1 >> 16) & 0xFF).astype(np.uint8)
    out["occ"][ok] = ((w1 >> 24) & 0xFF).astype(np.uint8).view(np.int8)
    return out


def geometry(n_bits, voxel_size, center=(0.0, 0.0, 0.0), eq=(0, 0, 0)):
    """a query_ref.Geometry without a map"""
    cfg = dict(x_n=n_bits[0], y_n=n_bits[1], z_n=n_bits[2], voxel_size=voxel_size)
    return qr.Geometry(cfg, dict(map_center=list(center), eq_steps=list(eq)))
