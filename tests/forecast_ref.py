"""NumPy restatement of the forecast (include/sdm.h: sdm_forecast_stamps / sdm_forecast_update / sdm_get_forecast /
sdm_get_forecast_cells / sdm_query_forecast / sdm_query_forecast_segments), for the tests.

Takes what a caller can read back from a map - voxels() and the query_ref.Geometry of its ring_state() and
configuration - plus the motions and horizons, and answers independently of the kernels:
  * stamps: the shift per track and horizon in float64 (np.rint: ties to even), the swept lines by the header's integer
    formula, ascending track, then horizon, then j;
  * field: the classes from the result array in map-index order, every source cell moved by every stamp of its track
    (np.bitwise_or.at / np.minimum.at), the info block, the list of marked cells;
  * point-time queries;
  * space-time segments: query_ref.query_segments' walk, extended by the parameters at which every cell is entered and
    left, plus a flag for segments on which such a time lies within TIME_AMBIGUOUS seconds of a horizon.
"""
import numpy as np

NOTHING = 0xFFFFFFFF
SHIFT_MAX = 1024
MAX_HORIZONS = 16
MAX_STAMPS = 65536
SWEPT = 1
TIME_AMBIGUOUS = 1e-6
MOTION = np.dtype([("track", "<u2"), ("pad", "<u2"), ("v", "<f4", (3,))])
STAMP = np.dtype([("track", "<u2"), ("horizon", "u1"), ("pad", "u1"), ("d", "<i2", (3,)), ("pad2", "<i2")])
CLS_UNKNOWN, CLS_FREE, CLS_STAYS, CLS_SOURCE = 0, 1, 2, 3


def motions(tracks, velocities):
    mo = np.zeros(len(tracks), MOTION)
    mo["track"] = tracks
    mo["v"] = np.asarray(velocities, np.float32).reshape(-1, 3)
    return mo


def shifts(voxel_size, v, horizons):
    """s[k][a] for one velocity: two float64 operations, ties to even, clamped"""
    v = np.asarray(v, np.float32).astype(np.float64)
    t = np.asarray(horizons, np.float32).astype(np.float64)
    s = np.rint((v[None, :] * t[:, None]) / np.float64(np.float32(voxel_size)))
    return np.clip(s, -SHIFT_MAX, SHIFT_MAX).astype(np.int64)


def swept_line(p, q):
    """the stamps of one horizon under SWEPT: from p (excluded) to q (included)"""
    D = q - p
    J = int(np.abs(D).max())
    if J == 0:
        return q[None, :].copy()
    j = np.arange(1, J + 1, dtype=np.int64)[:, None]
    return p[None, :] + np.sign(D)[None, :] * ((2 * j * np.abs(D)[None, :] + J) // (2 * J))


def stamps(voxel_size, mo, horizons, swept=False):
    """-> STAMP records in the order of the header (no limit on their number here)"""
    mo = np.asarray(mo, MOTION).reshape(-1)
    rows = []
    for i in np.argsort(mo["track"], kind="stable"):
        s = shifts(voxel_size, mo["v"][i], horizons)
        p = np.zeros(3, np.int64)
        for k in range(len(s)):
            line = swept_line(p, s[k]) if swept else s[k][None, :]
            for d in line:
                rows.append((int(mo["track"][i]), k, 0, tuple(int(x) for x in d), 0))
            p = s[k]
    return np.array(rows, STAMP) if rows else np.zeros(0, STAMP)


def grids(geo, voxels):
    """occ and track of every cell, indexed [z, y, x] in map coordinates"""
    g = geo.voxel_grid()
    return voxels["occ"][g], voxels["track"][g]


class Field:
    """mask and first [z, y, x], info (a dict), the horizons"""

    def __init__(self, geo, voxels, voxel_size, mo, horizons, swept=False, occ_track=None):
        mo = np.zeros(0, MOTION) if mo is None else np.asarray(mo, MOTION).reshape(-1)
        self.t = np.asarray(horizons, np.float32).reshape(-1)
        self.geo = geo
        occ, track = grids(geo, voxels) if occ_track is None else occ_track   # (grids() of the same map, computed once)
        in_table = np.isin(track, mo["track"])
        cls = np.where(occ == -1, CLS_UNKNOWN, np.where(occ == 0, CLS_FREE, np.where(in_table, CLS_SOURCE, CLS_STAYS))).astype(np.uint32)
        shape = cls.shape
        NZ, NY, NX = shape
        mask = (cls << 16).ravel()
        first = np.full(mask.size, NOTHING, np.uint32)
        st = stamps(voxel_size, mo, self.t, swept)
        n_in = n_out = 0
        src = cls == CLS_SOURCE
        for tr in np.unique(st["track"]):
            cells = np.argwhere(src & (track == tr))[:, ::-1].astype(np.int64)   # (x, y, z)
            mine = st[st["track"] == tr]
            if not len(cells):
                continue
            for s0 in range(0, len(mine), 256):
                part = mine[s0:s0 + 256]
                land = cells[None, :, :] + part["d"].astype(np.int64)[:, None, :]
                ok = ((land >= 0) & (land < np.array([NX, NY, NZ]))).all(axis=2)
                n_in += int(ok.sum())
                n_out += int((~ok).sum())
                k = np.broadcast_to(part["horizon"].astype(np.uint32)[:, None], ok.shape)[ok]
                w = (land[..., 0] + NX * (land[..., 1] + NY * land[..., 2]))[ok]
                np.bitwise_or.at(mask, w, np.uint32(1) << k)
                np.minimum.at(first, w, (k << 16) | np.uint32(tr))
        self.mask, self.first = mask.reshape(shape), first.reshape(shape)
        self.info = dict(n_motions=len(mo), n_horizons=len(self.t), n_stamps=len(st), flags=SWEPT if swept else 0, n_sources=int(src.sum()),
                         n_marked=int(((mask & 0xFFFF) != 0).sum()), n_marks_in=n_in, n_marks_out=n_out)

    def cells(self):
        """-> (cell, mask, first) of the marked cells, ascending cell word"""
        m, f = self.mask.ravel(), self.first.ravel()
        c = np.flatnonzero((m & 0xFFFF) != 0).astype(np.uint32)
        return c, m[c], f[c]

    def horizon(self, T):
        """the smallest k with T <= t[k], the last one beyond"""
        T = np.asarray(T, np.float64)
        return np.minimum((self.t.astype(np.float64)[None, :] < T[..., None]).sum(axis=-1), len(self.t) - 1)

    def query(self, xyzt):
        """-> dict of arrays like FORECAST_RESULT"""
        p = np.asarray(xyzt, np.float32).reshape(-1, 4)
        geo = self.geo
        u = geo.u(p[:, :3])
        with np.errstate(invalid="ignore"):
            ok = ((u >= 0) & (u < geo.N.astype(np.float32))).all(axis=1) & np.isfinite(p[:, 3])
        c = np.floor(np.where(ok[:, None], u, 0)).astype(np.int64)
        w = c[:, 0] + geo.N[0] * (c[:, 1] + geo.N[1] * c[:, 2])
        m, f = self.mask.ravel()[w], self.first.ravel()[w]
        k = self.horizon(np.where(ok, p[:, 3], 0).astype(np.float64))
        cls = (m >> 16) & 3
        bit = (m >> k.astype(np.uint32)) & 1
        state = np.where(cls == CLS_STAYS, 1, np.where(bit == 1, 2, np.where(cls == CLS_SOURCE, 3, np.where(cls == CLS_FREE, 0, -1))))
        none = f == NOTHING
        n = len(p)
        out = dict(state=np.full(n, -1, np.int8), horizon=np.full(n, 0xFF, np.uint8), track=np.zeros(n, np.uint16), mask=np.zeros(n, np.uint16),
                   first_horizon=np.full(n, 0xFF, np.uint8), pad=np.zeros(n, np.uint8))
        out["state"][ok] = state[ok]
        out["horizon"][ok] = k[ok]
        out["track"][ok] = np.where(none, 0, f & 0xFFFF)[ok]
        out["mask"][ok] = (m & 0xFFFF)[ok]
        out["first_horizon"][ok] = np.where(none, 0xFF, (f >> 16) & 0xFF)[ok]
        return out

    def query_segments(self, seg, unknown_blocks=False, vacated_blocks=False, record=False):
        """-> dict of arrays like FORECAST_HIT, plus time_ambiguous: a time at which a visited cell is entered or left lies
        within TIME_AMBIGUOUS of a horizon; with record=True also the walk of every segment, a list of (x, y, z)"""
        seg = np.asarray(seg, np.float32).reshape(-1, 8)
        geo = self.geo
        ua, ub = geo.u(seg[:, 0:3]), geo.u(seg[:, 4:7])
        ta, tb = seg[:, 3].astype(np.float64), seg[:, 7].astype(np.float64)
        n = len(ua)
        Nf = geo.N.astype(np.float32)
        with np.errstate(invalid="ignore"):
            finite = np.isfinite(ua).all(axis=1) & np.isfinite(ub).all(axis=1) & np.isfinite(ta) & np.isfinite(tb) & (ta <= tb)
        A = np.where(finite[:, None], ua, 0).astype(np.float64)
        D = np.where(finite[:, None], ub, 0).astype(np.float64) - A
        T0 = np.where(finite, ta, 0)
        dT = np.where(finite, tb, 0) - T0
        with np.errstate(invalid="ignore"):
            inside = finite & ((ua >= 0) & (ua < Nf)).all(axis=1)
            para_out = ((D == 0) & ~((ua >= 0) & (ua < Nf))).any(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0 = (0.0 - A) / D
            t1 = (geo.N - A) / D
        lo, hi = np.where(D != 0, np.minimum(t0, t1), -np.inf), np.where(D != 0, np.maximum(t0, t1), np.inf)
        t_in, t_out = lo.max(axis=1), hi.min(axis=1)
        clip_ok = finite & ~inside & ~para_out & (t_in <= 1) & (t_out > 0) & (t_in < t_out)
        out = dict(t=np.full(n, -1.0, np.float32), cell=np.full(n, NOTHING, np.uint32), cells=np.zeros(n, np.int32), track=np.zeros(n, np.uint16),
                   state=np.zeros(n, np.int8), horizon=np.full(n, 0xFF, np.uint8), time_ambiguous=np.zeros(n, bool))
        if unknown_blocks:
            out["t"][~inside] = 0.0      # non-finite, or a outside the map
            out["state"][~inside] = -1
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
        t64 = self.t.astype(np.float64)
        mask, first = self.mask.ravel(), self.first.ravel()
        while active.any():
            ids = rows[active]
            cc = c[ids]
            out["cells"][ids] += 1
            if record:
                for i, cell in zip(ids, cc):
                    walks[i].append(tuple(int(v) for v in cell))
            Ai, Di = A[ids], D[ids]
            with np.errstate(divide="ignore", invalid="ignore"):
                tn = np.where(Di > 0, (cc + 1 - Ai) / Di, np.where(Di < 0, (cc - Ai) / Di, np.inf))
            ax = np.argmin(tn, axis=1)                      # (the first of equal minima: x before y before z)
            tm = tn[np.arange(len(ids)), ax]
            end = tm > 1
            # when the cell is occupied, and the horizon bits of that time
            Tin, Tout = T0[ids] + t_cur[ids] * dT[ids], T0[ids] + np.where(end, 1.0, tm) * dT[ids]
            out["time_ambiguous"][ids] |= (np.abs(Tin[:, None] - t64[None, :]).min(axis=1) < TIME_AMBIGUOUS) | \
                                          (np.abs(Tout[:, None] - t64[None, :]).min(axis=1) < TIME_AMBIGUOUS)
            k_lo, k_hi = self.horizon(Tin).astype(np.uint32), self.horizon(Tout).astype(np.uint32)
            rng = ((np.uint32(2) << k_hi) - (np.uint32(1) << k_lo)).astype(np.uint32)
            w = cc[:, 0] + geo.N[0] * (cc[:, 1] + geo.N[1] * cc[:, 2])
            m = mask[w]
            cls, bits = (m >> 16) & 3, m & rng
            blocks = (cls == CLS_STAYS) | (bits != 0) | ((cls == CLS_UNKNOWN) & unknown_blocks) | ((cls == CLS_SOURCE) & vacated_blocks)
            h = ids[blocks]
            state = np.where(cls == CLS_STAYS, 1, np.where(bits != 0, 2, np.where(cls == CLS_SOURCE, 3, -1)))[blocks]
            out["t"][h] = t_cur[h]
            out["cell"][h] = w[blocks]
            out["state"][h] = state
            lowest = np.array([(int(b) & -int(b)).bit_length() - 1 for b in bits[blocks]], np.int64)
            out["horizon"][h] = np.where(state == 2, lowest, 0xFF)
            out["track"][h] = np.where(state == 2, first[w[blocks]] & 0xFFFF, 0)
            active[h] = False
            keep = ~blocks
            ids, ax, tm, end = ids[keep], ax[keep], tm[keep], end[keep]
            active[ids[end]] = False
            ids, ax, tm = ids[~end], ax[~end], tm[~end]
            c[ids, ax] += step[ids, ax]
            t_cur[ids] = tm
            cn = c[ids, ax]
            left = (cn < 0) | (cn >= geo.N[ax])
            active[ids[left]] = False
            if unknown_blocks:
                out["t"][ids[left]] = tm[left]
                out["state"][ids[left]] = -1
        return (out, walks) if record else out


def equal_fields(mask, first, info, ref):
    """None if the build equals the restatement, else what differs"""
    if not np.array_equal(mask, ref.mask):
        bad = np.argwhere(mask != ref.mask)
        return "mask differs at %d cells, first at [z, y, x] %s: %#x, want %#x" % (len(bad), bad[0], mask[tuple(bad[0])], ref.mask[tuple(bad[0])])
    if not np.array_equal(first, ref.first):
        bad = np.argwhere(first != ref.first)
        return "first differs at %d cells, first at [z, y, x] %s: %#x, want %#x" % (len(bad), bad[0], first[tuple(bad[0])], ref.first[tuple(bad[0])])
    for k, v in ref.info.items():
        if int(info[k]) != v:
            return "info.%s = %d, want %d" % (k, int(info[k]), v)
    return None


def equal_records(got, want, names):
    for k in names:
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero(got[k] != want[k])
            return "%s differs at %d items, first %d: %r, want %r" % (k, len(bad), bad[0], got[k][bad[0]], want[k][bad[0]])
    return None
