"""NumPy restatement of the world archive (include/sdm.h: sdm_world_update / sdm_get_world_info / sdm_get_world_bricks /
sdm_get_world_occupied / sdm_query_world_points / sdm_get_world_region / sdm_world_clear), for the tests.

Two models.  `Archive` is the brick model the header describes: a pool of bricks in creation order, 512 words and a
header each, a capacity, the candidates of an update ranked in brick order.  `Naive` is a dict from world cell to word
and knows nothing of bricks; tests/test_world_ref.py holds the first against the second.

merge() works on the [z, y, x] word grid esdf_ref.snapshot_grid returns (track | label << 16 | occ << 24 per map-index
cell) and the moved_steps of the ring state the grid was read under."""
import numpy as np

from semantic_dsp_map_amd import binding

UNKNOWN = 0xFF000000
STATIC_ONLY = binding.WORLD_STATIC_ONLY
OBSERVED_ONLY = binding.WORLD_OBSERVED_ONLY
ALL_FLAGS = [0, STATIC_ONLY, OBSERVED_ONLY, STATIC_ONLY | OBSERVED_ONLY]
B_MIN, B_MAX = -32768, 32767


def occ_of(words):
    return (np.asarray(words, np.uint32) >> 24).astype(np.uint8).view(np.int8)


def writes(words, max_movable, flags):
    """which cells of a word grid write under the flags"""
    w = np.asarray(words, np.uint32)
    occ, track = occ_of(w).astype(np.int32), (w & 0xFFFF).astype(np.int32)
    out = occ >= 0
    if flags & STATIC_ONLY:
        out &= ~((occ >= 1) & (track >= 1) & (track <= max_movable))
    if flags & OBSERVED_ONLY:
        out &= occ != 2
    return out


def default_max_bricks(N):
    want, p = max(2 * int(np.prod([int(n) // 8 + 1 for n in N])), 4096), 1
    while p < want:
        p <<= 1
    return p


def block_origin(snap, moved_steps):
    """world cell (x, y, z) of map-index cell (0, 0, 0)"""
    N = np.array(snap.shape[::-1], np.int64)
    return np.asarray(moved_steps, np.int64) - (N >> 1)


class Archive:
    def __init__(self, max_bricks):
        self.max_bricks = int(max_bricks)
        self.slot = {}                                   # (bx, by, bz) -> pool slot
        self.coord = []                                  # per pool slot
        self.cells = []                                  # per pool slot: 512 words in cell-word order
        self.first_stamp, self.last_stamp = [], []
        self.n_updates = self.created_last = self.dropped_last = self.out_of_range_last = self.dropped_total = 0
        self.flags = self.stamp = 0

    # ---- the getters' orders
    def order(self):
        """pool slots in brick order: ascending in (bz, by, bx)"""
        return sorted(range(len(self.coord)), key=lambda s: (self.coord[s][2], self.coord[s][1], self.coord[s][0]))

    def bricks(self):
        o = self.order()
        hdr = np.zeros(len(o), binding.WORLD_BRICK)
        cells = np.stack([self.cells[s] for s in o]) if len(o) else np.zeros((0, 512), np.uint32)
        occ = occ_of(cells)
        for k, s in enumerate(o):
            hdr[k]["bx"], hdr[k]["by"], hdr[k]["bz"] = self.coord[s]
            hdr[k]["first_stamp"], hdr[k]["last_stamp"] = self.first_stamp[s], self.last_stamp[s]
        hdr["n_occupied"], hdr["n_free"] = (occ >= 1).sum(axis=1), (occ == 0).sum(axis=1)
        return hdr, cells

    def info(self):
        out = np.zeros(1, binding.WORLD_INFO)[0]
        out["bmax"] = -1
        if not self.n_updates:
            return out
        hdr, _ = self.bricks()
        out["n_bricks"], out["max_bricks"], out["n_updates"] = len(hdr), self.max_bricks, self.n_updates
        out["created_last"], out["dropped_last"], out["out_of_range_last"] = self.created_last, self.dropped_last, self.out_of_range_last
        out["dropped_total"] = self.dropped_total
        out["n_occupied"], out["n_free"] = hdr["n_occupied"].astype(np.uint64).sum(), hdr["n_free"].astype(np.uint64).sum()
        if len(hdr):
            b = np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int32)
            out["bmin"], out["bmax"] = b.min(axis=0), b.max(axis=0)
        out["flags"], out["stamp"] = self.flags, self.stamp
        return out

    def occupied(self, voxel_size):
        """POINT list: ascending in (brick order, cell word); the min corner is (float32)g * voxel_size"""
        hdr, cells = self.bricks()
        k, w = np.nonzero(occ_of(cells) >= 1)
        out = np.zeros(len(k), binding.POINT)
        size = np.float32(voxel_size)
        for a, (name, b) in enumerate((("x", hdr["bx"]), ("y", hdr["by"]), ("z", hdr["bz"]))):
            g = b[k].astype(np.int64) * 8 + ((w >> (3 * a)) & 7)
            out[name] = g.astype(np.float32) * size
        word = cells[k, w]
        out["track"], out["label"], out["occ"] = word & 0xFFFF, (word >> 16) & 0xFF, occ_of(word)
        return out

    # ---- lookups
    def words_at(self, g):
        """-> (words, stamps) of world cells g (n, 3) int64: UNKNOWN and 0 where the archive has no brick"""
        g = np.asarray(g, np.int64).reshape(-1, 3)
        b, c = g >> 3, g & 7
        word = c[:, 0] | (c[:, 1] << 3) | (c[:, 2] << 6)
        words, stamps = np.full(len(g), UNKNOWN, np.uint32), np.zeros(len(g), np.uint32)
        off = np.int64(1) << 20                        # (one key per brick: sorting rows is slow)
        uniq, inv = np.unique(((b[:, 2] + off) << 42) | ((b[:, 1] + off) << 21) | (b[:, 0] + off), return_inverse=True)
        uniq = np.stack([(uniq & (2 * off - 1)) - off, ((uniq >> 21) & (2 * off - 1)) - off, (uniq >> 42) - off], 1)
        if not len(g) or not self.cells:
            return words, stamps
        slot = np.array([self.slot.get(key, -1) for key in map(tuple, uniq.tolist())], np.int64)[inv.reshape(-1)]
        have = slot >= 0
        words[have] = np.stack(self.cells)[slot[have], word[have]]
        stamps[have] = np.array(self.last_stamp, np.uint32)[slot[have]]
        return words, stamps

    def query_points(self, xyz, voxel_size):
        """WORLD_CELL per point: the cell is floorf(p * recip) per axis in float32"""
        p = np.asarray(xyz, np.float32).reshape(-1, 3)
        recip = np.float32(1.0) / np.float32(voxel_size)
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.floor(p * recip)
            ok = ((v >= np.float32(-262144.0)) & (v < np.float32(262144.0))).all(axis=1)
        g = np.where(ok[:, None], v, 0).astype(np.int64)
        out = np.zeros(len(p), binding.WORLD_CELL)
        out["occ"] = -1
        words, stamps = self.words_at(g[ok])
        out["track"][ok], out["label"][ok], out["occ"][ok], out["stamp"][ok] = words & 0xFFFF, (words >> 16) & 0xFF, occ_of(words), stamps
        return out

    def region(self, cell_min, size):
        """uint32 [sz, sy, sx]: the words of the box of world cells"""
        lo = np.asarray(cell_min, np.int64)
        z, y, x = np.meshgrid(*(np.arange(int(n), dtype=np.int64) for n in size[::-1]), indexing="ij")
        g = np.stack([x.ravel() + lo[0], y.ravel() + lo[1], z.ravel() + lo[2]], 1)
        out = np.full(len(g), UNKNOWN, np.uint32)
        b = g >> 3
        ok = ((b >= B_MIN) & (b <= B_MAX)).all(axis=1)
        out[ok] = self.words_at(g[ok])[0]
        return out.reshape(int(size[2]), int(size[1]), int(size[0]))


def brick_view(snap, moved_steps):
    """the block laid over the bricks it overlaps -> (b0 (x, y, z), nb (x, y, z), words [nc, 512]) with the candidates in
    brick order and the words in cell-word order; cells of a brick outside the block read UNKNOWN"""
    N = np.array(snap.shape[::-1], np.int64)
    g0 = block_origin(snap, moved_steps)
    b0 = g0 >> 3
    nb = ((g0 + N - 1) >> 3) - b0 + 1
    off = g0 - b0 * 8
    pad = np.full((int(nb[2]) * 8, int(nb[1]) * 8, int(nb[0]) * 8), UNKNOWN, np.uint32)
    pad[off[2]:off[2] + N[2], off[1]:off[1] + N[1], off[0]:off[0] + N[0]] = snap
    v = pad.reshape(int(nb[2]), 8, int(nb[1]), 8, int(nb[0]), 8).transpose(0, 2, 4, 1, 3, 5)
    return b0, nb, np.ascontiguousarray(v).reshape(-1, 512)


def merge(archive, snap, moved_steps, gts, max_movable, opt):
    """one sdm_world_update: opt is the flags word"""
    flags = int(opt)
    b0, nb, words = brick_view(np.asarray(snap, np.uint32), moved_steps)
    wr = writes(words, max_movable, flags)
    n_wr = wr.sum(axis=1)
    created = dropped = out_of_range = 0
    n_before = len(archive.coord)
    for c in np.nonzero(n_wr)[0].tolist():                   # ascending candidate index = brick order
        t, kx = divmod(c, int(nb[0]))
        kz, ky = divmod(t, int(nb[1]))
        key = (int(b0[0]) + kx, int(b0[1]) + ky, int(b0[2]) + kz)
        if not all(B_MIN <= v <= B_MAX for v in key):
            out_of_range += 1
            continue
        s = archive.slot.get(key)
        if s is None:
            if n_before + created >= archive.max_bricks:      # rank `created`... of the bricks that asked: no room
                dropped += int(n_wr[c])
                continue
            s = n_before + created
            created += 1
            archive.slot[key] = s
            archive.coord.append(key)
            archive.first_stamp.append(int(gts))
            archive.last_stamp.append(int(gts))
            archive.cells.append(np.full(512, UNKNOWN, np.uint32))
        archive.cells[s][wr[c]] = words[c][wr[c]]
        archive.last_stamp[s] = int(gts)
    archive.n_updates += 1
    archive.created_last, archive.dropped_last, archive.out_of_range_last = created, dropped, out_of_range
    archive.dropped_total += dropped
    archive.flags, archive.stamp = flags, int(gts)
    return archive


# ---- the naive model: world cell -> word
class Naive:
    def __init__(self):
        self.cell = {}

    def merge(self, snap, moved_steps, max_movable, flags, skip_bricks=()):
        """every writing cell stores its word; skip_bricks: bricks the capacity rule left out of this update"""
        snap = np.asarray(snap, np.uint32)
        g0 = block_origin(snap, moved_steps)
        z, y, x = np.nonzero(writes(snap, max_movable, flags))
        skip = set(skip_bricks)
        for i, j, k, w in zip((x + g0[0]).tolist(), (y + g0[1]).tolist(), (z + g0[2]).tolist(), snap[z, y, x].tolist()):
            if (i >> 3, j >> 3, k >> 3) not in skip:
                self.cell[(i, j, k)] = w

    def word(self, g):
        return self.cell.get(tuple(int(v) for v in g), UNKNOWN)

    def bricks(self):
        return sorted({(i >> 3, j >> 3, k >> 3) for i, j, k in self.cell}, key=lambda b: (b[2], b[1], b[0]))

    def occupied(self):
        """world cells with occ >= 1, ascending in (bz, by, bx, cell word)"""
        key = lambda g: (g[2] >> 3, g[1] >> 3, g[0] >> 3, (g[0] & 7) | (g[1] & 7) << 3 | (g[2] & 7) << 6)  # noqa: E731
        return sorted((g for g, w in self.cell.items() if 1 <= (w >> 24) < 128), key=key)
