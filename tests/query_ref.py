"""NumPy restatement of the batched map queries (include/sdm.h: sdm_query_points / _segments / _boxes), for the tests.

Takes what a caller can read back from a map - voxels(), ring_state() and the configuration - and answers the three
queries independently of the kernels:
  * points: the map's own float32 position -> storage index mapping, op for op (global_pos_to_voxel, with the PINNED
    cast that takes u in (-1, 0) to cell 0);
  * segments: the cell walk in float64 (crossings t = (plane - u_a) / (u_b - u_a)), vectorised over segments, plus an
    "ambiguous" flag for segments on which two plane crossings, or an end point and a plane, lie within 1e-3 voxel of
    each other (there float32 / float64 rounding may legitimately order them either way);
  * boxes: enumeration of the box's cells in map coordinates.
"""
import numpy as np

INVALID = 0xFFFFFFFF
AMBIGUOUS_VOXELS = 1e-3


class Geometry:
    def __init__(self, cfg, ring):
        self.n_bits = np.array([cfg["x_n"], cfg["y_n"], cfg["z_n"]])
        self.N = np.array([1 << int(b) for b in self.n_bits], np.int64)
        size = np.float32(cfg["voxel_size"])
        self.recip = np.float32(1.0) / size
        self.pmin = np.array([-(np.float32(int(N) >> 1) * size) for N in self.N], np.float32)
        self.center = np.array(ring["map_center"], np.float32)
        self.eq = np.array(ring["eq_steps"], np.int64)

    def u(self, p):
        """map-index coordinates (float32), ((p - center) - pmin) * recip"""
        p = np.asarray(p, np.float32).reshape(-1, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            return ((p - self.center) - self.pmin) * self.recip

    def voxel(self, c):
        """storage index of in-map cells c (n, 3) int: the per-axis ring correction, row-major storage"""
        c = np.asarray(c, np.int64).reshape(-1, 3)
        r = c + self.eq
        r = np.where(r < 0, r + self.N, np.where(r >= self.N, r - self.N, r))
        return ((r[:, 2] << (self.n_bits[0] + self.n_bits[1])) | (r[:, 1] << self.n_bits[0]) | r[:, 0]).astype(np.uint32)

    def voxel_grid(self):
        """storage index of every cell, indexed [z, y, x] in map coordinates"""
        z, y, x = np.meshgrid(*(np.arange(n) for n in self.N[::-1]), indexing="ij")
        return self.voxel(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)).reshape(tuple(self.N[::-1]))


def query_points(geo, voxels, xyz):
    """-> (VOXEL_RESULT array, storage indices) as the kernel must return them"""
    u = geo.u(xyz)
    with np.errstate(invalid="ignore"):
        ok = ((u > np.float32(-1)) & (u < geo.N.astype(np.float32))).all(axis=1)
    c = np.where(ok[:, None], u, 0).astype(np.int32)     # C's truncating cast, taken only where it is defined
    idx = np.full(len(u), INVALID, np.uint32)
    idx[ok] = geo.voxel(c[ok])
    out = np.empty(len(u), voxels.dtype)
    out["wsum"], out["track"], out["label"], out["occ"] = -1.0, 0, 0, -1
    out[ok] = voxels[idx[ok]]
    return out, idx


def segment_ambiguous(geo, a, b):
    """per segment: two plane crossings (planes 0..N of each axis), or an end point and such a plane, closer than
    AMBIGUOUS_VOXELS in voxel units along the segment"""
    ua, ub = geo.u(a).astype(np.float64), geo.u(b).astype(np.float64)
    n = len(ua)
    amb = ~np.isfinite(ua).all(axis=1) | ~np.isfinite(ub).all(axis=1)
    for s0 in range(0, n, 4096):
        A, B = ua[s0:s0 + 4096], ub[s0:s0 + 4096]
        D = B - A
        L = np.sqrt((D * D).sum(axis=1))
        fin = np.isfinite(L)
        A, D, L = np.where(fin[:, None], A, 0), np.where(fin[:, None], D, 0), np.where(fin, L, 0)
        eps = np.where(L > 0, AMBIGUOUS_VOXELS / np.maximum(L, 1e-300), np.inf)
        ts = [np.zeros((len(A), 1)), np.ones((len(A), 1))]
        for ax in range(3):
            k = np.arange(int(geo.N[ax]) + 1, dtype=np.float64)[None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (k - A[:, ax:ax + 1]) / D[:, ax:ax + 1]
                t = np.where(np.isfinite(t) & (t >= -eps[:, None]) & (t <= 1 + eps[:, None]), t, np.nan)
            ts.append(t)
            # a zero-length (or axis-parallel) segment: its end point near a plane of this axis
            near = np.abs(k - A[:, ax:ax + 1]).min(axis=1) < AMBIGUOUS_VOXELS
            amb[s0:s0 + len(A)] |= near & (D[:, ax] == 0)
        t = np.sort(np.concatenate(ts, axis=1), axis=1)     # (NaN last)
        with np.errstate(invalid="ignore"):
            gaps = np.diff(t, axis=1) * L[:, None]
            gap = np.where(np.isnan(gaps), np.inf, gaps).min(axis=1)
        amb[s0:s0 + len(A)] |= (L > 0) & (gap < AMBIGUOUS_VOXELS)   # (a zero-length segment: only its point near a plane)
        amb[s0:s0 + len(A)] |= ~fin
    return amb


def query_segments(geo, voxels, a, b, unknown_blocks=False, record=False):
    """-> SEGMENT_HIT-like dict of arrays (t, voxel, cells, track, label, occ); with record=True also the walk of every
    segment: a list of in-map cells (x, y, z) in visiting order (the walk without any cell blocking if voxels is None)"""
    ua, ub = geo.u(a), geo.u(b)
    n = len(ua)
    Nf = geo.N.astype(np.float32)
    finite = np.isfinite(ua).all(axis=1) & np.isfinite(ub).all(axis=1)
    A = np.where(finite[:, None], ua, 0).astype(np.float64)
    D = np.where(finite[:, None], ub, 0).astype(np.float64) - A
    inside = finite & ((ua >= 0) & (ua < Nf)).all(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (0.0 - A) / D
        t1 = (geo.N - A) / D
    lo, hi = np.where(D != 0, np.minimum(t0, t1), -np.inf), np.where(D != 0, np.maximum(t0, t1), np.inf)
    para_out = ((D == 0) & ~((ua >= 0) & (ua < Nf))).any(axis=1)
    t_in, t_out = lo.max(axis=1), hi.min(axis=1)
    clip_ok = finite & ~inside & ~para_out & (t_in <= 1) & (t_out > 0) & (t_in < t_out)

    out = dict(t=np.full(n, -1.0, np.float32), voxel=np.full(n, INVALID, np.uint32), cells=np.zeros(n, np.int32),
               track=np.zeros(n, np.uint16), label=np.zeros(n, np.uint8), occ=np.full(n, -1, np.int8))
    if unknown_blocks:
        out["t"][~inside] = 0.0      # non-finite, or a outside the map
        active = inside.copy()
    else:
        active = inside | clip_ok
    t_cur = np.where(inside, 0.0, np.maximum(t_in, 0.0))
    with np.errstate(invalid="ignore"):
        c_clip = np.clip(np.floor(A + t_cur[:, None] * D), 0, geo.N - 1)
    c = np.where(inside[:, None], np.floor(np.where(finite[:, None], ua, 0)), np.where(active[:, None], c_clip, 0)).astype(np.int64)
    step = np.sign(D).astype(np.int64)
    walks = [[] for _ in range(n)] if record else None
    rows = np.arange(n)
    while active.any():
        ids = rows[active]
        cc = c[ids]
        out["cells"][ids] += 1
        if record:
            for i, cell in zip(ids, cc):
                walks[i].append(tuple(int(v) for v in cell))
        if voxels is not None:
            v = geo.voxel(cc)
            occ = voxels["occ"][v]
            blocks = (occ >= 1) | ((occ == -1) & unknown_blocks)
            h = ids[blocks]
            out["t"][h] = t_cur[h]
            out["voxel"][h] = v[blocks]
            for k in ("track", "label", "occ"):
                out[k][h] = voxels[k][v[blocks]]
            active[h] = False
            ids, cc = ids[~blocks], cc[~blocks]
        Ai, Di = A[ids], D[ids]
        with np.errstate(divide="ignore", invalid="ignore"):
            tn = np.where(Di > 0, (cc + 1 - Ai) / Di, np.where(Di < 0, (cc - Ai) / Di, np.inf))
        ax = np.argmin(tn, axis=1)                      # (the first of equal minima: x before y before z)
        tm = tn[np.arange(len(ids)), ax]
        end = tm > 1
        active[ids[end]] = False
        ids, ax, tm = ids[~end], ax[~end], tm[~end]
        c[ids, ax] += step[ids, ax]
        t_cur[ids] = tm
        cn = c[ids, ax]
        left = (cn < 0) | (cn >= geo.N[ax])
        active[ids[left]] = False
        if unknown_blocks:
            out["t"][ids[left]] = tm[left]
    return (out, walks) if record else out


def query_boxes(geo, voxels, lo, hi):
    """-> BOX_RESULT-like dict of arrays"""
    ulo, uhi = geo.u(lo), geo.u(hi)
    lo, hi = np.asarray(lo, np.float32).reshape(-1, 3), np.asarray(hi, np.float32).reshape(-1, 3)
    n = len(ulo)
    occ_grid = voxels["occ"][geo.voxel_grid()]
    vox_grid = geo.voxel_grid()
    out = dict(n_occupied=np.zeros(n, np.int32), n_free=np.zeros(n, np.int32), n_unknown=np.zeros(n, np.int32),
               first_occupied=np.full(n, INVALID, np.uint32), clipped=np.zeros(n, np.int32))
    with np.errstate(invalid="ignore"):
        valid = (np.isfinite(lo) & np.isfinite(hi) & (lo <= hi)).all(axis=1)
        flo, fhi = np.floor(ulo), np.floor(uhi)
    for i in np.flatnonzero(valid):
        out["clipped"][i] = int((flo[i] < 0).any() or (fhi[i] >= geo.N).any())
        a = np.maximum(flo[i], 0)
        e = np.minimum(fhi[i], geo.N - 1)
        if (a > e).any():
            continue
        a, e = a.astype(np.int64), e.astype(np.int64)
        sl = (slice(a[2], e[2] + 1), slice(a[1], e[1] + 1), slice(a[0], e[0] + 1))
        o = occ_grid[sl]
        out["n_occupied"][i] = int((o >= 1).sum())
        out["n_free"][i] = int((o == 0).sum())
        out["n_unknown"][i] = int((o == -1).sum())
        if out["n_occupied"][i]:
            out["first_occupied"][i] = int(vox_grid[sl][o >= 1].min())
    return out


def box_cells_meshgrid(geo, lo, hi):
    """the cells of one box (x, y, z), by brute force over the whole map: every cell whose index range overlaps"""
    ulo, uhi = geo.u(lo)[0], geo.u(hi)[0]
    z, y, x = np.meshgrid(*(np.arange(n) for n in geo.N[::-1]), indexing="ij")
    cells = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    keep = ((cells >= np.floor(ulo)) & (cells <= np.floor(uhi))).all(axis=1)
    return cells[keep]
