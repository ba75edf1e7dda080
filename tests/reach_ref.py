"""NumPy / heapq restatement of the travel-cost field (include/sdm.h: sdm_reach_update / sdm_get_reach / sdm_query_reach /
sdm_reach_paths), for the tests.  No SciPy.

Grids are indexed [z, y, x] in map-index order; a cell word is the flat index of that grid.  From what a caller can read
back - voxels(), ring_state() through tests/query_ref.Geometry, the configuration - or from a block directly it gives:
  * the traversable grid of a frame, or of a distance field's snapshot with a clearance;
  * per cell the bit mask of its allowed moves, from shifted ANDs over the block padded with non-traversable cells;
  * the cost field by a heap Dijkstra truncated at max_cost, and by whole-grid Bellman-Ford sweeps to the fixed point
    (the second is for small blocks: the tests hold the first to it);
  * the descent by the pinned rule, the paths, the query results and the info block.
"""
import heapq

import numpy as np

from semantic_dsp_map_amd.binding import REACH_INFO, REACH_RESULT
from tests import esdf_ref as er

NO_COST = 0xFFFFFFFF
FACE_CONNECTED = 0x1
THROUGH_UNKNOWN = 0x2
MOVES = [n for n in range(27) if n != 13]


def move_offset(n):
    """(dx, dy, dz) of move n"""
    return n % 3 - 1, (n // 3) % 3 - 1, n // 9 - 1


def move_weight(n):
    return {1: 10, 2: 14, 3: 17}[sum(1 for d in move_offset(n) if d)]


FACE_MOVES = [n for n in MOVES if move_weight(n) == 10]
assert FACE_MOVES == [4, 10, 12, 14, 16, 22]


def occ_grid(geo, voxels):
    return voxels["occ"][geo.voxel_grid()]


def traversable(occ, through_unknown=False):
    """occ [z, y, x] int8 -> bool"""
    return (occ == 0) | ((occ == -1) if through_unknown else False)


def traversable_of_field(snap, d2, min_d2, through_unknown=False):
    """the distance field's snapshot words and d2 [z, y, x] -> bool: the class from the word, and d2 >= min_d2"""
    occ = ((snap >> 24) & 0xFF).astype(np.uint8).view(np.int8)
    return traversable(occ, through_unknown) & (d2.astype(np.int64) >= int(min_d2))


def _shifted(padded, shape, s):
    """the padded block read at offset s = (sx, sy, sz) from every cell"""
    NZ, NY, NX = shape
    return padded[1 + s[2]:1 + s[2] + NZ, 1 + s[1]:1 + s[1] + NY, 1 + s[0]:1 + s[0] + NX]


def allowed_bits(trav, face_connected=False):
    """-> uint32 [z, y, x]: bit n set where move n is allowed from the cell: every cell c + s, s_a in {0, o_a}, inside
    the block and traversable"""
    padded = np.pad(trav, 1, constant_values=False)
    out = np.zeros(trav.shape, np.uint32)
    for n in (FACE_MOVES if face_connected else MOVES):
        o = move_offset(n)
        ok = np.ones(trav.shape, bool)
        for k in range(8):
            s = tuple(o[a] if (k >> a) & 1 else 0 for a in range(3))
            ok &= _shifted(padded, trav.shape, s)
        out |= ok.astype(np.uint32) << np.uint32(n)
    return out


def _flat_moves(shape, face_connected):
    NZ, NY, NX = shape
    return [(n, move_offset(n)[0] + NX * (move_offset(n)[1] + NY * move_offset(n)[2]), move_weight(n))
            for n in (FACE_MOVES if face_connected else MOVES)]


def start_words(trav, words):
    """the distinct usable start cells: inside the block and traversable"""
    w = np.unique(np.asarray(words, np.int64).reshape(-1))
    w = w[(w >= 0) & (w < trav.size)]
    return w[trav.ravel()[w]]


def dijkstra(trav, starts, face_connected=False, max_cost=0, allowed=None):
    """cost uint32 [z, y, x] from the start cell words (usable ones: start_words) by a binary heap"""
    allowed = allowed_bits(trav, face_connected) if allowed is None else allowed
    al = allowed.ravel().tolist()
    moves = _flat_moves(trav.shape, face_connected)
    limit = int(max_cost) if max_cost else NO_COST - 1
    cost = [NO_COST] * trav.size
    heap = []
    for s in start_words(trav, starts).tolist():
        cost[s] = 0
        heap.append((0, s))
    heapq.heapify(heap)
    pop, push = heapq.heappop, heapq.heappush
    while heap:
        d, c = pop(heap)
        if d > cost[c]:
            continue
        a = al[c]
        for n, off, w in moves:
            if (a >> n) & 1:
                nd = d + w
                if nd < cost[c + off] and nd <= limit:
                    cost[c + off] = nd
                    push(heap, (nd, c + off))
    return np.array(cost, np.uint32).reshape(trav.shape)


def bellman_ford(trav, starts, face_connected=False, max_cost=0):
    """the same field as the fixed point of whole-grid sweeps (for small blocks)"""
    allowed = allowed_bits(trav, face_connected)
    inf = np.int64(1) << 40
    cost = np.full(trav.shape, inf, np.int64)
    cost.ravel()[start_words(trav, starts)] = 0
    limit = int(max_cost) if max_cost else NO_COST - 1
    while True:
        padded = np.pad(cost, 1, constant_values=inf)
        new = cost.copy()
        for n in (FACE_MOVES if face_connected else MOVES):
            cand = _shifted(padded, trav.shape, move_offset(n)) + move_weight(n)
            ok = ((allowed >> np.uint32(n)) & 1).astype(bool) & (cand <= limit)
            new = np.where(ok & (cand < new), cand, new)
        if np.array_equal(new, cost):
            break
        cost = new
    return np.where(cost >= inf, np.int64(NO_COST), cost).astype(np.uint32)


def components(trav, face_connected=False):
    """-> int64 [z, y, x]: per traversable cell the smallest cell word it is connected to by allowed moves, -1 elsewhere
    (min-hooking and pointer jumping over the edge list, as tests/frontiers_ref.py labels its cells)"""
    allowed = allowed_bits(trav, face_connected).ravel()
    ea, eb = [], []
    for n, off, _ in _flat_moves(trav.shape, face_connected):
        if off > 0:   # (the rule is symmetric: every edge once)
            src = np.flatnonzero((allowed >> np.uint32(n)) & 1)
            ea.append(src), eb.append(src + off)
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    parent = np.arange(trav.size, dtype=np.int64)
    while True:
        pa, pb = parent[ea], parent[eb]
        open_ = pa != pb
        if not open_.any():
            break
        ea, eb, pa, pb = ea[open_], eb[open_], pa[open_], pb[open_]
        lo = np.minimum(pa, pb)
        np.minimum.at(parent, pa, lo)
        np.minimum.at(parent, pb, lo)
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    return np.where(trav.ravel(), parent, -1).reshape(trav.shape)


class Field:
    """a built field: trav, allowed and cost [z, y, x], and what the info block holds"""

    def __init__(self, trav, starts, face_connected=False, through_unknown=False, min_d2=0, max_cost=0):
        self.trav = trav
        self.shape = trav.shape
        self.face = bool(face_connected)
        self.allowed = allowed_bits(trav, self.face)
        self.cost = dijkstra(trav, starts, self.face, max_cost, self.allowed)
        self.flags = (FACE_CONNECTED if face_connected else 0) | (THROUGH_UNKNOWN if through_unknown else 0)
        reached = self.cost != NO_COST
        self.info = np.zeros(1, REACH_INFO)[0]
        self.info["n_starts_used"] = len(start_words(trav, starts))
        self.info["n_traversable"] = int(trav.sum())
        self.info["n_reached"] = int(reached.sum())
        self.info["max_cost_reached"] = int(self.cost[reached].max()) if reached.any() else 0
        self.info["flags"], self.info["min_d2"], self.info["max_cost"] = self.flags, int(min_d2), int(max_cost)
        self._moves = _flat_moves(self.shape, self.face)

    # ---- descent
    def next_move(self, c):
        """(n, next cell word) of the first descent step from cell word c with 0 < cost < NO_COST"""
        cost, al = self.cost.ravel(), int(self.allowed.ravel()[c])
        for n, off, w in self._moves:   # ascending n
            if (al >> n) & 1 and int(cost[c + off]) != NO_COST and int(cost[c + off]) + w == int(cost[c]):
                return n, c + off
        raise AssertionError("no descent step from cell %d (cost %d)" % (c, int(cost[c])))

    def path(self, c):
        """the cell words from c to a start, both included; [] where c has no cost"""
        cost = self.cost.ravel()
        if c < 0 or c >= cost.size or int(cost[c]) == NO_COST:
            return []
        out = [int(c)]
        while int(cost[c]) != 0:
            _, c = self.next_move(c)
            out.append(int(c))
        return out

    # ---- goals
    def goal_words(self, geo=None, xyz=None, cells=None):
        """per goal its cell word, NO_COST outside the map / non-finite"""
        if cells is not None:
            w = np.asarray(cells, np.int64).reshape(-1)
            return np.where((w >= 0) & (w < self.cost.size), w, NO_COST)
        u = geo.u(xyz)
        with np.errstate(invalid="ignore"):
            ok = ((u >= 0) & (u < geo.N.astype(np.float32))).all(axis=1)
        c = np.floor(np.where(ok[:, None], u, 0)).astype(np.int64)
        NZ, NY, NX = self.shape
        return np.where(ok, c[:, 0] + NX * (c[:, 1] + NY * c[:, 2]), NO_COST)

    def query(self, voxel_size, geo=None, xyz=None, cells=None):
        words = self.goal_words(geo, xyz, cells)
        out = np.zeros(len(words), REACH_RESULT)
        out["cost"], out["metres"], out["cell"], out["next"], out["status"] = NO_COST, -1.0, words.astype(np.uint32), 255, 3
        cost, trav = self.cost.ravel(), self.trav.ravel()
        scale = np.float32(voxel_size) * np.float32(0.1)
        for i, c in enumerate(words.tolist()):
            if c == NO_COST:
                continue
            if not trav[c]:
                out["status"][i] = 2
            elif int(cost[c]) == NO_COST:
                out["status"][i] = 1
            else:
                out["status"][i] = 0
                out["cost"][i] = cost[c]
                out["metres"][i] = np.float32(cost[c]) * scale
                out["next"][i] = 13 if int(cost[c]) == 0 else self.next_move(c)[0]
        return out

    def paths(self, geo=None, xyz=None, cells=None):
        """-> list of int arrays, one per goal"""
        return [np.array(self.path(c) if c != NO_COST else [], np.int64) for c in self.goal_words(geo, xyz, cells).tolist()]


def field_of_map(geo, voxels, starts, **kw):
    """the field of a frame: geo, voxels() and start cell words"""
    return Field(traversable(occ_grid(geo, voxels), kw.get("through_unknown", False)), starts, **kw)


def field_of_esdf(geo, voxels, max_movable, esdf_flags, starts, min_d2, **kw):
    """the field over a distance field's snapshot (built from geo, voxels under esdf_flags) with clearance min_d2"""
    snap = er.snapshot_grid(geo, voxels)
    d2 = er.edt_d2(er.obstacle_grid(geo, voxels, max_movable, esdf_flags))
    return Field(traversable_of_field(snap, d2, min_d2, kw.get("through_unknown", False)), starts, min_d2=min_d2, **kw)


def words_of_points(geo, xyz):
    """cell words of global positions (NO_COST outside / non-finite)"""
    u = geo.u(xyz)
    with np.errstate(invalid="ignore"):
        ok = ((u >= 0) & (u < geo.N.astype(np.float32))).all(axis=1)
    c = np.floor(np.where(ok[:, None], u, 0)).astype(np.int64)
    return np.where(ok, c[:, 0] + geo.N[0] * (c[:, 1] + geo.N[1] * c[:, 2]), NO_COST)


def cell_centres(geo, voxel_size, words):
    """the global positions of the centres of cell words (float32)"""
    w = np.asarray(words, np.int64)
    NX, NY = int(geo.N[0]), int(geo.N[1])
    c = np.stack([w % NX, (w // NX) % NY, w // (NX * NY)], axis=1).astype(np.float32)
    return ((geo.center + geo.pmin) + (c + np.float32(0.5)) * np.float32(voxel_size)).astype(np.float32)


def equal_results(got, want):
    """None if two REACH_RESULT arrays are equal on every field, metres by its bit pattern; else what differs"""
    if len(got) != len(want):
        return "length %d != %d" % (len(got), len(want))
    for k in REACH_RESULT.names:
        x, y = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            bad = np.flatnonzero(x != y)
            return "%s differs at goals %s: %s / %s" % (k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    return None


def equal_all(got_cost, got_info, ref):
    """the cost field and the info block (all but `rounds`) against a Field; None or what differs"""
    if got_cost.shape != ref.cost.shape:
        return "shape %s != %s" % (got_cost.shape, ref.cost.shape)
    if not np.array_equal(got_cost, ref.cost):
        bad = np.flatnonzero(got_cost.ravel() != ref.cost.ravel())
        return "cost differs at %d cells, first %s: %s / %s" % (len(bad), bad[:5], got_cost.ravel()[bad[:5]], ref.cost.ravel()[bad[:5]])
    for k in REACH_INFO.names:
        if k != "rounds" and int(got_info[k]) != int(ref.info[k]):
            return "info.%s: %d != %d" % (k, int(got_info[k]), int(ref.info[k]))
    return None


def check_path(field, path):
    """a descended path ends at a start, strictly decreases, uses allowed moves only and is short enough (None or a message)"""
    cost, al = field.cost.ravel(), field.allowed.ravel()
    NZ, NY, NX = field.shape
    if not len(path):
        return "empty"
    if int(cost[path[-1]]) != 0:
        return "does not end at a start"
    if len(path) > int(cost[path[0]]) // 10 + 1:
        return "longer than cost / 10 + 1"
    by_off = {off: (n, w) for n, off, w in field._moves}
    for a, b in zip(path[:-1], path[1:]):
        if b - a not in by_off:
            return "step %d -> %d is no move" % (a, b)
        n, w = by_off[b - a]
        if not (int(al[a]) >> n) & 1:
            return "move %d from %d is not allowed" % (n, a)
        if int(cost[b]) + w != int(cost[a]) or int(cost[b]) >= int(cost[a]):
            return "cost does not fall by the move's weight at %d" % a
    return None
