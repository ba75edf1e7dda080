"""NumPy restatement of the world distance field (include/sdm.h: sdm_world_esdf_update / sdm_get_world_esdf /
sdm_query_world_distance), for the tests.  No SciPy.  Written twice:

  * BrickModel: per archived brick eight 64-bit obstacle words (bit cx + 8 cy); per field brick the words of the
    (2 H + 1)^3 bricks round it, H = 1 for R <= 8 and 2 beyond (an absent brick: zeros, or ones under unknown_is_obstacle),
    and three truncated passes.  x works on the layer words by shifts - the cell t to the left is bit - t, the columns
    that would wrap into the next row masked out and the neighbour brick's columns shifted in; y and z are windowed minima
    over - R .. R, scanned ascending and replaced only by a strictly smaller sum.  A candidate whose partial sum exceeds R^2
    is dropped at once.  `wrap_mask=False` leaves the column masks out, `halo=` overrides H, `descending=True` scans the
    other way (and prefers the right on a tie in x): what the tests show such a model to get wrong.
  * CellModel: per field brick a dense boolean grid of the brick and a margin of R cells, filled from a dict of the archive's
    bricks; every cell takes the first offset of the ball, in ascending (d2, dz, dy, dx) order, that lands on an obstacle.

Both take what a caller can read back - world_bricks() - and give coords, d2, offset and the info block;
tests/test_world_esdf_ref.py holds one to the other, tests/test_world_esdf_gpu.py the library to BrickModel.  World cells
are (x, y, z); brick = cell >> 3; a brick's cell word is cx | cy << 3 | cz << 6; offset is (dx, dy, dz)."""
import numpy as np

from semantic_dsp_map_amd.binding import (WORLD_DISTANCE_RESULT, WORLD_ESDF_BOX, WORLD_ESDF_FAR, WORLD_ESDF_INFO, WORLD_ESDF_NONE,
                                          WORLD_ESDF_STATIC_ONLY, WORLD_ESDF_UNKNOWN_IS_OBSTACLE)

B_MIN, B_MAX = -32768, 32767
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
COL = 0x0101010101010101
NO_DX, NO_D2 = 127, 1 << 20


def occ_of(words):
    return ((np.asarray(words, np.uint32) >> 24) & 0xFF).astype(np.uint8).view(np.int8)


def flags_of(unknown_is_obstacle=False, static_only=False, box=None):
    return ((WORLD_ESDF_UNKNOWN_IS_OBSTACLE if unknown_is_obstacle else 0) | (WORLD_ESDF_STATIC_ONLY if static_only else 0) |
            (WORLD_ESDF_BOX if box is not None else 0))


def brick_coords(hdr):
    coord = np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int64).reshape(-1, 3)
    order = np.lexsort((coord[:, 0], coord[:, 1], coord[:, 2]))
    assert np.array_equal(order, np.arange(len(coord))), "world_bricks() is in brick order"
    return coord


def in_box(coord, box):
    if box is None:
        return np.ones(len(coord), bool)
    return ((coord >= np.asarray(box[0], np.int64)) & (coord <= np.asarray(box[1], np.int64))).all(axis=1).reshape(-1)


def obstacles(cells, max_movable, unknown_is_obstacle, static_only):
    """bool [n, 512]: the obstacle cells of the archived words"""
    words = np.asarray(cells, np.uint32).reshape(-1, 512)
    occ, track = occ_of(words), (words & 0xFFFF).astype(np.int64)
    movable = (track >= 1) & (track <= max_movable)
    return ((occ >= 1) & ~(movable if static_only else False)) | ((occ == -1) if unknown_is_obstacle else False)


class _Common:
    def _finish(self, coords, d2, off, radius, flags, stamp):
        n = len(coords)
        self.coords = np.asarray(coords, np.int64).reshape(-1, 3).astype(np.int16)
        d2 = np.asarray(d2, np.int64).reshape(n, 512)
        none = d2 > radius * radius
        self.d2 = np.where(none, WORLD_ESDF_NONE, d2).astype(np.uint16)
        self.offset = np.where(none[..., None], 0, np.asarray(off, np.int64).reshape(n, 512, 3)).astype(np.int8)
        self.radius = int(radius)
        self.info = np.zeros(1, WORLD_ESDF_INFO)[0]
        self.info["n_bricks"], self.info["flags"], self.info["radius"], self.info["stamp"] = n, flags, radius, stamp
        self.info["n_obstacle_cells"], self.info["n_near_cells"] = int((self.d2 == 0).sum()), int((~none).sum())

    def query(self, cells, voxel_size):
        """WORLD_DISTANCE_RESULT per world cell of `cells` (n, 3)"""
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        size = np.float32(voxel_size)
        rank = {tuple(b): r for r, b in enumerate(self.coords.astype(np.int64).tolist())}
        out = np.zeros(len(cells), WORLD_DISTANCE_RESULT)
        for i, c in enumerate(cells.tolist()):
            out[i]["cell"] = out[i]["nearest"] = c
            r = rank.get((c[0] >> 3, c[1] >> 3, c[2] >> 3))
            if r is None:
                out[i]["d2"], out[i]["distance"] = 0xFFFFFFFF, -1.0
                continue
            w = (c[0] & 7) | (c[1] & 7) << 3 | (c[2] & 7) << 6
            v = int(self.d2[r, w])
            if v == WORLD_ESDF_NONE:
                out[i]["d2"], out[i]["distance"] = WORLD_ESDF_FAR, np.sqrt(np.float32(self.radius * self.radius + 1)) * size
            else:
                out[i]["d2"], out[i]["distance"] = v, np.sqrt(np.float32(v)) * size
                out[i]["nearest"] = np.asarray(c) + self.offset[r, w].astype(np.int64)
        return out


def layer_words(mask):
    """bool [n, 512] -> uint64 [n, 8]: bit cx + 8 cy of layer cz"""
    m = np.asarray(mask, bool).reshape(-1, 8, 64)
    return (m.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


def cols_below(t):
    return np.uint64(COL * ((1 << t) - 1))


def cols_from(t):
    return np.uint64(COL * (0xFF & ~((1 << t) - 1)))


def bits_of(words):
    """uint64 [...] -> bool [..., 8 (cy), 8 (cx)]"""
    b = np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")
    return b.reshape(words.shape + (8, 8)).view(bool)


class BrickModel(_Common):
    def __init__(self, hdr, cells, radius, max_movable, unknown_is_obstacle=False, static_only=False, box=None, stamp=0, wrap_mask=True,
                 halo=None, descending=False):
        R = int(radius)
        assert 1 <= R <= 16
        H = (1 if R <= 8 else 2) if halo is None else int(halo)
        W, S = 2 * H + 1, 8 * (2 * H + 1)
        coord = brick_coords(hdr)
        obst = layer_words(obstacles(cells, max_movable, unknown_is_obstacle, static_only))
        place = {tuple(b): j for j, b in enumerate(coord.tolist())}       # the whole archive
        field = np.flatnonzero(in_box(coord, box))
        n = len(field)
        absent = ALL if unknown_is_obstacle else np.uint64(0)
        # the words of the neighbourhood: A[r, bz, by, bx, layer]
        A = np.full((n, W, W, W, 8), absent, np.uint64)
        for r, j in enumerate(field.tolist()):
            b = coord[j].tolist()
            for oz in range(-H, H + 1):
                for oy in range(-H, H + 1):
                    for ox in range(-H, H + 1):
                        q = (b[0] + ox, b[1] + oy, b[2] + oz)
                        k = place.get(q) if all(B_MIN <= v <= B_MAX for v in q) else None
                        if k is not None:
                            A[r, oz + H, oy + H, ox + H] = obst[k]
        zero = np.zeros((n, W, W, 8), np.uint64)

        def word_at(o):   # the words of the brick column at x offset o of the brick's own; beyond the halo there is nothing
            return A[:, :, :, o + H, :] if -H <= o <= H else zero

        # ---- x, on the layer words: bit (cx, cy) of left[t] / right[t] says "the cell t to the left / right is an obstacle"
        dx = np.full((n, W, W, 8, 8, 8), NO_DX, np.int8)      # [r, bz, by, layer, cy, cx]
        for t in range(R, -1, -1):                             # the nearest is written last
            a, b = divmod(t, 8)
            lo, hi = (cols_below(b), cols_from(b)) if wrap_mask else (ALL, ALL)
            lo2, hi2 = (cols_from(8 - b), cols_below(8 - b)) if wrap_mask else (ALL, ALL)
            left = (word_at(-a) << np.uint64(b)) & hi
            right = (word_at(a) >> np.uint64(b)) & hi2
            if b:
                left = left | ((word_at(-a - 1) >> np.uint64(8 - b)) & lo)
                right = right | ((word_at(a + 1) << np.uint64(8 - b)) & lo2)
            first, second = ((right, t), (left, -t)) if not descending else ((left, -t), (right, t))
            for w, v in (first, second):                       # (ascending: the left one, the smaller x, wins the tie)
                np.putmask(dx, bits_of(w), v)
        # dense from here: [r, z, y, cx] over the halo's S x S rows
        dx = dx.transpose(0, 1, 3, 2, 4, 5).reshape(n, S, S, 8)
        lo_c, order = 8 * H, (range(R, -R - 1, -1) if descending else range(-R, R + 1))
        R2 = R * R
        # ---- y: per (z, cy, cx) of the brick's columns, the windowed minimum of dx^2 + dy^2
        d_y = np.full((n, S, 8, 8), NO_D2, np.int64)
        o_y = np.zeros((2, n, S, 8, 8), np.int64)              # dx, dy of the candidate kept
        for k in order:
            y0, y1 = lo_c + k, lo_c + k + 8
            if y0 < 0 or y1 > S:
                continue                                        # (only with halo= too small: beyond the halo there is nothing)
            cand = dx[:, :, y0:y1, :].astype(np.int64)
            v = np.where(cand == NO_DX, NO_D2, cand * cand + k * k)
            take = (v <= R2) & (v < d_y)
            np.copyto(d_y, v, where=take)
            np.copyto(o_y[0], cand, where=take)
            np.copyto(o_y[1], k, where=take)
        # ---- z
        d_z = np.full((n, 8, 8, 8), NO_D2, np.int64)
        o_z = np.zeros((3, n, 8, 8, 8), np.int64)
        for k in order:
            z0, z1 = lo_c + k, lo_c + k + 8
            if z0 < 0 or z1 > S:
                continue
            cand = d_y[:, z0:z1]
            v = np.where(cand >= NO_D2, NO_D2, cand + k * k)
            take = (v <= R2) & (v < d_z)
            np.copyto(d_z, v, where=take)
            np.copyto(o_z[0], o_y[0][:, z0:z1], where=take)
            np.copyto(o_z[1], o_y[1][:, z0:z1], where=take)
            np.copyto(o_z[2], k, where=take)
        o_z = np.moveaxis(o_z, 0, -1)
        self._finish(coord[field], d_z.reshape(n, 512), o_z.reshape(n, 512, 3), R, flags_of(unknown_is_obstacle, static_only, box), stamp)


def ball_offsets(R):
    """the offsets (dx, dy, dz) with |o|^2 <= R^2 in ascending (d2, dz, dy, dx) order"""
    ax = np.arange(-R, R + 1)
    dz, dy, dx = np.meshgrid(ax, ax, ax, indexing="ij")
    d2 = dx * dx + dy * dy + dz * dz
    keep = d2 <= R * R
    o = np.stack([dx[keep], dy[keep], dz[keep], d2[keep]], 1)
    return o[np.lexsort((o[:, 0], o[:, 1], o[:, 2], o[:, 3]))]


class CellModel(_Common):
    def __init__(self, hdr, cells, radius, max_movable, unknown_is_obstacle=False, static_only=False, box=None, stamp=0):
        R = int(radius)
        T = 8 + 2 * R
        coord = brick_coords(hdr)
        solid = obstacles(cells, max_movable, unknown_is_obstacle, static_only).reshape(-1, 8, 8, 8)   # [j, cz, cy, cx]
        place = {tuple(b): j for j, b in enumerate(coord.tolist())}
        field = np.flatnonzero(in_box(coord, box))
        n = len(field)
        grid = np.full((n, T, T, T), bool(unknown_is_obstacle))       # [r, z, y, x]; cell (0, 0, 0) of the brick at (R, R, R)
        reach = -((-R) // 8)                                          # bricks the margin reaches into
        for r, j in enumerate(field.tolist()):
            b = coord[j].tolist()
            for oz in range(-reach, reach + 1):
                for oy in range(-reach, reach + 1):
                    for ox in range(-reach, reach + 1):
                        q = (b[0] + ox, b[1] + oy, b[2] + oz)
                        k = place.get(q) if all(B_MIN <= v <= B_MAX for v in q) else None
                        if k is None:
                            continue
                        lo = [R + 8 * o for o in (ox, oy, oz)]        # where the neighbour's cell 0 falls in the grid, per axis
                        s = [slice(max(v, 0), min(v + 8, T)) for v in lo]
                        c = [slice(sl.start - v, sl.stop - v) for sl, v in zip(s, lo)]
                        grid[r, s[2], s[1], s[0]] = solid[k][c[2], c[1], c[0]]
        d2 = np.full((n, 512), NO_D2, np.int64)
        off = np.zeros((n, 512, 3), np.int64)
        w = np.arange(512)
        at = np.stack(np.broadcast_arrays(np.arange(n)[:, None], (w >> 6)[None] + R, ((w >> 3) & 7)[None] + R, (w & 7)[None] + R), -1).reshape(-1, 4)
        todo = np.arange(n * 512)
        flat_d2, flat_off = d2.reshape(-1), off.reshape(-1, 3)
        for dx, dy, dz, dd in ball_offsets(R).tolist():
            if not len(todo):
                break
            p = at[todo]
            hit = grid[p[:, 0], p[:, 1] + dz, p[:, 2] + dy, p[:, 3] + dx]
            if hit.any():
                found = todo[hit]
                flat_d2[found] = dd
                flat_off[found] = (dx, dy, dz)
                todo = todo[~hit]
        self._finish(coord[field], d2, off, R, flags_of(unknown_is_obstacle, static_only, box), stamp)


def difference(got, want):
    """None, or what differs between two (coords, d2, offset, info) answers - models or the library's getter"""
    for name, a, b in zip(("coords", "d2", "offset", "info"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            return "%s: shape / dtype %s %s against %s %s" % (name, a.shape, a.dtype, b.shape, b.dtype)
        if a.tobytes() != b.tobytes():
            if a.dtype.names:
                bad = [f for f in a.dtype.names if a[f].tobytes() != b[f].tobytes()]
                return "%s: fields %s differ: %s against %s" % (name, bad, a[bad[0]], b[bad[0]])
            at = np.argwhere(a != b)
            return "%s: %d entries differ, first at %s: %s against %s" % (name, len(at), at[0], a[tuple(at[0])], b[tuple(at[0])])
    return None


def answer(model):
    return model.coords, model.d2, model.offset, model.info
