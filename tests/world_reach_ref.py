"""NumPy / heapq restatement of world reach (include/sdm.h: sdm_world_reach_update / sdm_get_world_reach /
sdm_query_world_reach / sdm_world_reach_paths), for the tests.  No SciPy.  Written twice:

  * DenseField: the bricks of the field fall into groups of bricks that touch (26-neighbourhood of brick coordinates);
    nothing - no move, no inflation - crosses between two groups, because both stop at a cell of no brick.  Each group's
    bounding box becomes a dense [z, y, x] array in which the cells of no brick are not traversable, the inflation is
    plain shifts of the obstacle array, and the result goes through tests/reach_ref.py as it stands: its allowed_bits,
    its dijkstra, its Field.next_move and Field.path.
  * SparseField: a dict from world cell to class, cell by cell: its own allowed test over set lookups, its own heap
    Dijkstra, its own descent.

Both take what a caller can read back - world_bricks() - and give the getter's rows, the info block, the query results
and the paths; tests/test_world_reach_ref.py holds one to the other, tests/test_world_reach_gpu.py the library to them.
World cells are (x, y, z) int; brick = cell >> 3; a brick's cell word is cx | cy << 3 | cz << 6."""
import heapq
import itertools

import numpy as np

from semantic_dsp_map_amd.binding import (WORLD_REACH_BOX, WORLD_REACH_FACE_CONNECTED, WORLD_REACH_IGNORE_MOVABLE, WORLD_REACH_INFO,
                                          WORLD_REACH_RESULT, WORLD_REACH_THROUGH_UNKNOWN)
from tests import reach_ref as rr

NO_COST = rr.NO_COST
B_MIN, B_MAX = -32768, 32767


def occ_of(words):
    return ((np.asarray(words, np.uint32) >> 24) & 0xFF).astype(np.uint8).view(np.int8)


def flags_of(face_connected=False, through_unknown=False, ignore_movable=False, box=None):
    return ((WORLD_REACH_FACE_CONNECTED if face_connected else 0) | (WORLD_REACH_THROUGH_UNKNOWN if through_unknown else 0) |
            (WORLD_REACH_IGNORE_MOVABLE if ignore_movable else 0) | (WORLD_REACH_BOX if box is not None else 0))


def classes(cells, max_movable, through_unknown=False, ignore_movable=False):
    """words [n, 512] -> (traversable, obstacle) bool [n, 512], before any inflation"""
    cells = np.asarray(cells, np.uint32)
    occ, track = occ_of(cells).astype(np.int64), (cells & 0xFFFF).astype(np.int64)
    if ignore_movable:
        occ = np.where((occ >= 1) & (track >= 1) & (track <= max_movable), 0, occ)
    return (occ == 0) | ((occ == -1) if through_unknown else False), occ >= 1


def field_rows(hdr, box=None):
    """the rows of world_bricks() that belong to the field, in brick order (world_bricks() is in brick order already: the
    sort is stable and only asserts it)"""
    coord = np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int64).reshape(-1, 3)
    order = np.lexsort((coord[:, 0], coord[:, 1], coord[:, 2]))
    assert np.array_equal(order, np.arange(len(coord))), "world_bricks() is in brick order"
    keep = np.ones(len(coord), bool)
    if box is not None:
        keep = ((coord >= np.asarray(box[0], np.int64)) & (coord <= np.asarray(box[1], np.int64))).all(axis=1)
    return np.flatnonzero(keep), coord[keep]


def cells_of_points(xyz, voxel_size):
    """-> (world cells int64 [n, 3], ok): floorf(p * recip) per axis in float32; not ok - and (0, 0, 0) - for a point that is
    non-finite or beyond the brick range"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    recip = np.float32(1.0) / np.float32(voxel_size)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.floor(p * recip)
        ok = ((v >= np.float32(-262144.0)) & (v < np.float32(262144.0))).all(axis=1)
    return np.where(ok[:, None], v, 0).astype(np.int64), ok


def cells_in_range(cells):
    g = np.asarray(cells, np.int64).reshape(-1, 3)
    return g, (((g >> 3) >= B_MIN) & ((g >> 3) <= B_MAX)).all(axis=1)


def cell_centres(cells, voxel_size):
    return ((np.asarray(cells, np.int64).astype(np.float32) + np.float32(0.5)) * np.float32(voxel_size)).astype(np.float32)


class _Common:
    """what both restatements answer from cost_of / trav_of / has_brick / step: rows, info, queries, paths"""

    def _finish(self, coord, max_movable, inflate, max_cost, flags, stamp, n_starts_used):
        self.coords = coord.astype(np.int16).reshape(-1, 3)
        n = len(coord)
        self.cost = np.full((n, 512), NO_COST, np.uint32)
        self.trav = np.zeros((n, 512), bool)
        cz, cy, cx = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
        local = np.stack([cx.ravel(), cy.ravel(), cz.ravel()], 1)
        for r in range(n):
            g = coord[r] * 8 + local
            self.cost[r] = self.costs_of(g)
            self.trav[r] = self.travs_of(g)
        reached = self.cost != NO_COST
        self.info = np.zeros(1, WORLD_REACH_INFO)[0]
        self.info["n_bricks"], self.info["n_starts_used"] = n, n_starts_used
        self.info["n_traversable"], self.info["n_reached"] = int(self.trav.sum()), int(reached.sum())
        self.info["max_cost_reached"] = int(self.cost[reached].max()) if reached.any() else 0
        self.info["flags"], self.info["inflate"], self.info["max_cost"], self.info["stamp"] = flags, inflate, max_cost, stamp

    def goal_cells(self, voxel_size, xyz=None, cells=None):
        return cells_of_points(xyz, voxel_size) if cells is None else cells_in_range(cells)

    def query(self, voxel_size, xyz=None, cells=None):
        g, ok = self.goal_cells(voxel_size, xyz, cells)
        out = np.zeros(len(g), WORLD_REACH_RESULT)
        out["cost"], out["metres"], out["cell"], out["next"], out["status"] = NO_COST, -1.0, g.astype(np.int32), 255, 3
        scale = np.float32(voxel_size) * np.float32(0.1)
        for i, c in enumerate(map(tuple, g.tolist())):
            if not ok[i] or not self.has_brick(c):
                continue
            cost = self.cost_of(c)
            if not self.trav_of(c):
                out["status"][i] = 2
            elif cost == NO_COST:
                out["status"][i] = 1
            else:
                out["status"][i], out["cost"][i] = 0, cost
                out["metres"][i] = np.float32(cost) * scale
                out["next"][i] = 13 if cost == 0 else self.step(c)[0]
        return out

    def path(self, c):
        """the world cells from c to a start, both included; empty where c has no cost"""
        if not self.has_brick(c) or self.cost_of(c) == NO_COST:
            return np.zeros((0, 3), np.int64)
        out = [c]
        while self.cost_of(c) != 0:
            c = self.step(c)[1]
            out.append(c)
        return np.array(out, np.int64)

    def paths(self, voxel_size, xyz=None, cells=None):
        g, ok = self.goal_cells(voxel_size, xyz, cells)
        return [self.path(c) if ok[i] else np.zeros((0, 3), np.int64) for i, c in enumerate(map(tuple, g.tolist()))]


# ---- (a) dense, through tests/reach_ref.py ------------------------------------------------------------------------------
def _groups(coord):
    """the bricks in groups that touch: -> list of index arrays"""
    at = {tuple(c): i for i, c in enumerate(coord.tolist())}
    seen, out = set(), []
    for c0 in at:
        if c0 in seen:
            continue
        seen.add(c0)
        todo, group = [c0], []
        while todo:
            c = todo.pop()
            group.append(at[c])
            for d in itertools.product((-1, 0, 1), repeat=3):
                q = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
                if q in at and q not in seen:
                    seen.add(q)
                    todo.append(q)
        out.append(np.array(sorted(group), np.int64))
    return out


def _dilate(obst, r):
    """obst [z, y, x] bool -> the cells within Chebyshev distance r of an obstacle (shifts of the padded array)"""
    padded = np.pad(obst, r, constant_values=False)
    out = np.zeros(obst.shape, bool)
    Z, Y, X = obst.shape
    for dz, dy, dx in itertools.product(range(-r, r + 1), repeat=3):
        out |= padded[r + dz:r + dz + Z, r + dy:r + dy + Y, r + dx:r + dx + X]
    return out


class DenseField(_Common):
    def __init__(self, hdr, cells, start_cells, max_movable, inflate=0, max_cost=0, face_connected=False, through_unknown=False,
                 ignore_movable=False, box=None, stamp=0):
        rows, coord = field_rows(hdr, box)
        trav, obst = classes(np.asarray(cells, np.uint32).reshape(-1, 512)[rows], max_movable, through_unknown, ignore_movable)
        starts, ok = cells_in_range(start_cells)
        starts = starts[ok]
        self.parts, self.part_of = [], {}
        used = 0
        for group in _groups(coord):
            lo = coord[group].min(axis=0)
            size = (coord[group].max(axis=0) - lo + 1) * 8
            t, o = np.zeros(tuple(size[::-1]), bool), np.zeros(tuple(size[::-1]), bool)
            for r in group:
                x, y, z = (coord[r] - lo) * 8
                t[z:z + 8, y:y + 8, x:x + 8] = trav[r].reshape(8, 8, 8)
                o[z:z + 8, y:y + 8, x:x + 8] = obst[r].reshape(8, 8, 8)
                self.part_of[tuple(coord[r].tolist())] = len(self.parts)
            if inflate:
                t &= ~_dilate(o, inflate)
            s = starts - lo * 8
            s = s[((s >= 0) & (s < size)).all(axis=1)]
            words = s[:, 0] + size[0] * (s[:, 1] + size[1] * s[:, 2])
            field = rr.Field(t, words, face_connected=face_connected, max_cost=max_cost)
            used += int(field.info["n_starts_used"])
            self.parts.append((lo * 8, size, field))
        self._finish(coord, max_movable, inflate, max_cost, flags_of(face_connected, through_unknown, ignore_movable, box), stamp, used)

    def _word(self, c):
        lo, size, field = self.parts[self.part_of[(c[0] >> 3, c[1] >> 3, c[2] >> 3)]]
        return field, lo, size, int((c[0] - lo[0]) + size[0] * ((c[1] - lo[1]) + size[1] * (c[2] - lo[2])))

    def has_brick(self, c):
        return (c[0] >> 3, c[1] >> 3, c[2] >> 3) in self.part_of

    def cost_of(self, c):
        field, _, _, w = self._word(c)
        return int(field.cost.ravel()[w])

    def trav_of(self, c):
        field, _, _, w = self._word(c)
        return bool(field.trav.ravel()[w])

    def costs_of(self, g):
        lo, size, field = self.parts[self.part_of[tuple((g[0] >> 3).tolist())]]
        q = g - lo
        return field.cost[q[:, 2], q[:, 1], q[:, 0]]

    def travs_of(self, g):
        lo, size, field = self.parts[self.part_of[tuple((g[0] >> 3).tolist())]]
        q = g - lo
        return field.trav[q[:, 2], q[:, 1], q[:, 0]]

    def step(self, c):
        field, lo, size, w = self._word(c)
        n, nw = field.next_move(w)
        return n, (int(lo[0] + nw % size[0]), int(lo[1] + (nw // size[0]) % size[1]), int(lo[2] + nw // (size[0] * size[1])))


# ---- (b) sparse, cell by cell ---------------------------------------------------------------------------------------------
class SparseField(_Common):
    def __init__(self, hdr, cells, start_cells, max_movable, inflate=0, max_cost=0, face_connected=False, through_unknown=False,
                 ignore_movable=False, box=None, stamp=0):
        rows, coord = field_rows(hdr, box)
        words = np.asarray(cells, np.uint32).reshape(-1, 512)[rows]
        self.bricks = set(map(tuple, coord.tolist()))
        self.free, blocked = set(), set()
        for r, (bx, by, bz) in enumerate(coord.tolist()):
            for w, word in enumerate(words[r].tolist()):
                occ = (word >> 24) & 0xFF
                occ = occ - 256 if occ >= 128 else occ
                track = word & 0xFFFF
                if ignore_movable and occ >= 1 and 1 <= track <= max_movable:
                    occ = 0
                c = (bx * 8 + (w & 7), by * 8 + ((w >> 3) & 7), bz * 8 + (w >> 6))
                if occ == 0 or (through_unknown and occ == -1):
                    self.free.add(c)
                elif occ >= 1 and inflate:
                    for d in itertools.product(range(-inflate, inflate + 1), repeat=3):
                        blocked.add((c[0] + d[0], c[1] + d[1], c[2] + d[2]))
        self.free -= blocked
        self.moves = [(n, rr.move_offset(n), rr.move_weight(n)) for n in (rr.FACE_MOVES if face_connected else rr.MOVES)]
        limit = int(max_cost) if max_cost else NO_COST - 1
        self.dist, heap = {}, []
        g, ok = cells_in_range(start_cells)
        for s in set(map(tuple, g[ok].tolist())):
            if s in self.free:
                self.dist[s] = 0
                heap.append((0, s))
        used = len(heap)
        heapq.heapify(heap)
        while heap:
            d, c = heapq.heappop(heap)
            if d > self.dist[c]:
                continue
            for n, o, w in self.moves:
                if d + w <= limit and self.allowed(c, o):
                    q = (c[0] + o[0], c[1] + o[1], c[2] + o[2])
                    if d + w < self.dist.get(q, NO_COST):
                        self.dist[q] = d + w
                        heapq.heappush(heap, (d + w, q))
        self._finish(coord, max_movable, inflate, max_cost, flags_of(face_connected, through_unknown, ignore_movable, box), stamp, used)

    def allowed(self, c, o):
        """every cell c + s, s_a in {0, o_a}, is a traversable cell of the field"""
        for sx in {0, o[0]}:
            for sy in {0, o[1]}:
                for sz in {0, o[2]}:
                    if (c[0] + sx, c[1] + sy, c[2] + sz) not in self.free:
                        return False
        return True

    def has_brick(self, c):
        return (c[0] >> 3, c[1] >> 3, c[2] >> 3) in self.bricks

    def cost_of(self, c):
        return self.dist.get(tuple(c), NO_COST)

    def trav_of(self, c):
        return tuple(c) in self.free

    def costs_of(self, g):
        return np.array([self.dist.get(c, NO_COST) for c in map(tuple, g.tolist())], np.uint32)

    def travs_of(self, g):
        return np.array([c in self.free for c in map(tuple, g.tolist())], bool)

    def step(self, c):
        for n, o, w in self.moves:   # ascending n
            q = (c[0] + o[0], c[1] + o[1], c[2] + o[2])
            if self.allowed(c, o) and q in self.dist and self.dist[q] + w == self.dist[c]:
                return n, q
        raise AssertionError("no descent step from cell %s (cost %d)" % (c, self.dist[c]))


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def equal_results(got, want):
    """None if two WORLD_REACH_RESULT arrays are equal on every field, metres by its bit pattern; else what differs"""
    if len(got) != len(want):
        return "length %d != %d" % (len(got), len(want))
    for k in WORLD_REACH_RESULT.names:
        x, y = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            bad = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))
            return "%s differs at goals %s: %s / %s" % (k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    return None


def equal_fields(got, want):
    """two fields - restatements, or (coords, cost, info) of the getter against one - on rows and info without `rounds`"""
    g_coords, g_cost, g_info = (got.coords, got.cost, got.info) if isinstance(got, _Common) else got
    if g_coords.shape != want.coords.shape or not np.array_equal(g_coords, want.coords):
        return "coords differ: %s / %s" % (g_coords[:4].tolist(), want.coords[:4].tolist())
    if not np.array_equal(g_cost, want.cost):
        bad = np.argwhere(g_cost != want.cost)
        return "cost differs at %d cells, first (brick, word) %s: %s / %s" % (len(bad), bad[:4].tolist(), g_cost[tuple(bad[0])], want.cost[tuple(bad[0])])
    for k in WORLD_REACH_INFO.names:
        if k != "rounds" and int(g_info[k]) != int(want.info[k]):
            return "info.%s: %d != %d" % (k, int(g_info[k]), int(want.info[k]))
    return None
