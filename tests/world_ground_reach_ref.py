"""Restatement of world ground reach (include/sdm.h: sdm_world_ground_reach_update / sdm_get_world_ground_reach /
sdm_query_world_ground_reach / sdm_world_ground_reach_paths), for the tests.  No SciPy.  Written twice, from what a caller
can read back of the ground layer - coords, cells, d2 and the ground build's options (world_ground() or a model of
tests/world_ground_ref.py):

  * DenseReach: the tiles of the field in groups of touching tiles, each group as one dense 2-D array [v, u] with a margin
    of one column; the allowed bits of all eight moves as shifted array expressions; a heapq Dijkstra per group; the
    descent on the arrays.
  * SparseReach: a dictionary column -> (level, penalised) of the traversable columns alone; its own allowed test, column
    by column; label-correcting with a plain queue, no heap; its own descent.

Both give the costs, the info block (without `rounds`), query results and paths; tests/test_world_ground_reach_ref.py
holds one to the other, tests/test_world_ground_reach_gpu.py the library to SparseReach.  A move is k = (dv + 1) * 3 +
(du + 1); a tile's column word is cu | cv << 3."""
import heapq
from collections import deque

import numpy as np

from semantic_dsp_map_amd.binding import (WORLD_GROUND_NONE, WORLD_GROUND_REACH_BOX, WORLD_GROUND_REACH_FACE_CONNECTED,
                                          WORLD_GROUND_REACH_INFO, WORLD_GROUND_REACH_OPTIONS, WORLD_GROUND_REACH_RESULT)

C_MIN, C_MAX = -262144, 262143
B_MIN, B_MAX = -32768, 32767
NO_COST = 0xFFFFFFFF
NO_LEVEL = 0xFFFF
MOVES = [(k, k % 3 - 1, k // 3 - 1) for k in range(9) if k != 4]          # (number, du, dv), ascending in the number


def options_of(min_d2=0, soft_d2=0, penalty=0, max_climb=0, max_cost=0, face_connected=False, box=None):
    """the WORLD_GROUND_REACH_OPTIONS record SdmMap.world_ground_reach_update hands to the library"""
    o = np.zeros(1, WORLD_GROUND_REACH_OPTIONS)[0]
    o["flags"] = (WORLD_GROUND_REACH_FACE_CONNECTED if face_connected else 0) | (WORLD_GROUND_REACH_BOX if box is not None else 0)
    o["min_d2"], o["soft_d2"], o["penalty"], o["max_climb"], o["max_cost"] = min_d2, soft_d2, penalty, max_climb, max_cost
    if box is not None:
        o["tmin"], o["tmax"] = box[0], box[1]
    return o


def weight(du, dv):
    return 14 if du and dv else 10


class _Common:
    """what both restatements do alike: which tiles belong, the layout of the answers"""

    def _setup(self, coords, cells, d2, ground_options, starts, stamp, kw):
        self.o = options_of(**kw)
        self.start_cells = np.asarray(starts, np.int64).reshape(-1, 3)
        self.g = ground_options
        flags = int(self.o["flags"])
        self.face = bool(flags & WORLD_GROUND_REACH_FACE_CONNECTED)
        self.moves = [m for m in MOVES if not (self.face and m[1] and m[2])]
        a = int(self.g["up_axis"])
        self.a, self.au, self.av = a, (1 if a == 0 else 0), (1 if a == 2 else 2)
        self.sign, self.h_lo = int(self.g["up_sign"]), int(self.g["h_lo"])
        R = int(self.g["radius"])
        assert int(self.o["min_d2"]) <= R * R + 1 and int(self.o["soft_d2"]) <= R * R + 1
        self.budget = int(self.o["max_cost"]) or 0xFFFFFFFE
        self.penalty, self.climb = int(self.o["penalty"]), int(self.o["max_climb"])
        coords = np.asarray(coords, np.int64).reshape(-1, 2)
        keep = np.ones(len(coords), bool)
        if flags & WORLD_GROUND_REACH_BOX:
            lo, hi = np.asarray(self.o["tmin"], np.int64), np.asarray(self.o["tmax"], np.int64)
            keep = ((coords >= lo) & (coords <= hi)).all(axis=1)
        self.coords = coords[keep].astype(np.int16)
        cells, d2 = np.asarray(cells)[keep], np.asarray(d2)[keep].astype(np.int64)
        self.level = cells["level"].astype(np.int64)                    # [tile, column word]
        cls = cells["cls"].astype(np.int64)
        self.trav = ((cls & 3) == 1) & ((cls & 8) == 0) & ((d2 == WORLD_GROUND_NONE) | (d2 >= int(self.o["min_d2"])))
        self.pen = np.where((d2 != WORLD_GROUND_NONE) & (d2 < int(self.o["soft_d2"])), self.penalty, 0)
        self.rank = {tuple(t): r for r, t in enumerate(self.coords.astype(np.int64).tolist())}
        self.stamp = stamp

    def _start_columns(self, starts):
        out = []
        for g in np.asarray(starts, np.int64).reshape(-1, 3).tolist():
            if all(C_MIN <= v <= C_MAX for v in g):
                out.append((g[self.au], g[self.av]))
        return out

    def _finish(self, cost, n_starts_used):
        """cost: [tile, 64] Python-int costs of the unbounded field, None where there is no way"""
        n = len(self.coords)
        self.cost = np.full((n, 64), NO_COST, np.uint32)
        for r in range(n):
            for w in range(64):
                c = cost[r][w]
                if c is not None and c <= self.budget:
                    self.cost[r, w] = c
        reached = self.cost != NO_COST
        self.info = np.zeros(1, WORLD_GROUND_REACH_INFO)[0]
        self.info["n_tiles"], self.info["n_starts_used"], self.info["n_traversable"] = n, n_starts_used, int(self.trav.sum())
        self.info["n_reached"], self.info["max_cost_reached"] = int(reached.sum()), int(self.cost[reached].max()) if reached.any() else 0
        self.info["stamp"], self.info["options"] = self.stamp, self.o

    def where(self, iu, iv):
        """(tile rank, column word) of a column, or None"""
        r = self.rank.get((iu >> 3, iv >> 3))
        return None if r is None else (r, (iu & 7) | (iv & 7) << 3)

    def query(self, cells, voxel_size):
        """WORLD_GROUND_REACH_RESULT per world cell of `cells` (n, 3)"""
        size = np.float32(voxel_size)
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        out = np.zeros(len(cells), WORLD_GROUND_REACH_RESULT)
        out["cost"], out["metres"], out["level"], out["next"], out["status"] = NO_COST, -1.0, NO_LEVEL, 255, 3
        for i, g in enumerate(cells.tolist()):
            if not all(C_MIN <= v <= C_MAX for v in g):
                continue
            iu, iv = g[self.au], g[self.av]
            out[i]["col"] = (iu, iv)
            at = self.where(iu, iv)
            if at is None:
                continue
            out[i]["level"] = self.level[at]
            c = int(self.cost[at])
            out[i]["status"] = 2 if not self.trav[at] else 1 if c == NO_COST else 0
            if out[i]["status"] == 0:
                out[i]["cost"], out[i]["metres"] = c, np.float32(c) * (size * np.float32(0.1))
                out[i]["next"] = 4 if c == 0 else self.step(iu, iv)
        return out

    def cell_of(self, iu, iv):
        """the world cell the robot's base stands in on column (iu, iv)"""
        h = self.h_lo + int(self.level[self.where(iu, iv)]) + 1
        g = [0, 0, 0]
        g[self.a], g[self.au], g[self.av] = (h if self.sign > 0 else -1 - h), iu, iv
        return g

    def paths(self, cells, max_len, fill):
        """(rows int32 [n, max_len, 3], lens int32 [n]) as SdmMap.world_ground_reach_paths gives them"""
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        rows, lens = np.full((len(cells), max_len, 3), fill, np.int32), np.zeros(len(cells), np.int32)
        for i, g in enumerate(cells.tolist()):
            if not all(C_MIN <= v <= C_MAX for v in g):
                continue
            iu, iv = g[self.au], g[self.av]
            at = self.where(iu, iv)
            if at is None or int(self.cost[at]) == NO_COST:
                continue
            n = 0
            while True:
                if n < max_len:
                    rows[i, n] = self.cell_of(iu, iv)
                n += 1
                if int(self.cost[self.where(iu, iv)]) == 0:
                    break
                k = self.step(iu, iv)
                assert k != 255
                iu, iv = iu + k % 3 - 1, iv + k // 3 - 1
            lens[i] = n
        return rows, lens


# ---- the first restatement -------------------------------------------------------------------------------------------
class DenseReach(_Common):
    def __init__(self, coords, cells, d2, ground_options, starts, stamp=0, **kw):
        self._setup(coords, cells, d2, ground_options, starts, stamp, kw)
        tiles = [tuple(t) for t in self.coords.astype(np.int64).tolist()]
        # groups of tiles that touch with a side or a corner
        group_of, groups = {}, []
        for t in tiles:
            if t in group_of:
                continue
            members, todo = [], [t]
            group_of[t] = len(groups)
            while todo:
                q = todo.pop()
                members.append(q)
                for du in (-1, 0, 1):
                    for dv in (-1, 0, 1):
                        nq = (q[0] + du, q[1] + dv)
                        if nq in self.rank and nq not in group_of:
                            group_of[nq] = len(groups)
                            todo.append(nq)
            groups.append(members)
        self.group_of, self.grids = group_of, []
        cost = [[None] * 64 for _ in tiles]
        start_cols = self._start_columns(starts)
        used = set()
        for gi, members in enumerate(groups):
            u0, v0 = 8 * min(t[0] for t in members) - 1, 8 * min(t[1] for t in members) - 1
            nu, nv = 8 * max(t[0] for t in members) + 9 - u0, 8 * max(t[1] for t in members) + 9 - v0
            trav, level, pen = np.zeros((nv, nu), bool), np.zeros((nv, nu), np.int64), np.zeros((nv, nu), np.int64)
            for t in members:
                r = self.rank[t]
                sl = (slice(8 * t[1] - v0, 8 * t[1] - v0 + 8), slice(8 * t[0] - u0, 8 * t[0] - u0 + 8))
                trav[sl], level[sl], pen[sl] = self.trav[r].reshape(8, 8), self.level[r].reshape(8, 8), self.pen[r].reshape(8, 8)
            # allowed[k][v, u]: may the column make move k?  The margin is never traversable, so np.roll's wrap is harmless.
            allowed = {}
            sh = lambda a, du, dv: np.roll(a, (-dv, -du), axis=(0, 1))  # noqa: E731    a[v + dv, u + du] at [v, u]
            for k, du, dv in self.moves:
                parts = [(0, 0), (du, dv)] + ([(du, 0), (0, dv)] if du and dv else [])
                ok = np.ones((nv, nu), bool)
                hi, lo = np.full((nv, nu), -1, np.int64), np.full((nv, nu), 1 << 20, np.int64)
                for pu, pv in parts:
                    ok &= sh(trav, pu, pv)
                    hi, lo = np.maximum(hi, sh(level, pu, pv)), np.minimum(lo, sh(level, pu, pv))
                allowed[k] = ok & (hi - lo <= self.climb)
            dist = {}
            heap = []
            for iu, iv in start_cols:
                if group_of.get((iu >> 3, iv >> 3)) == gi and trav[iv - v0, iu - u0]:
                    used.add((iu, iv))
                    if (iv - v0, iu - u0) not in dist:
                        dist[(iv - v0, iu - u0)] = 0
                        heap.append((0, iv - v0, iu - u0))
            heapq.heapify(heap)
            done = set()
            while heap:
                c, y, x = heapq.heappop(heap)
                if (y, x) in done:
                    continue
                done.add((y, x))
                for k, du, dv in self.moves:
                    if allowed[k][y, x]:
                        q = (y + dv, x + du)
                        nc = c + weight(du, dv) + int(pen[q])
                        if nc < dist.get(q, 1 << 62):
                            dist[q] = nc
                            heapq.heappush(heap, (nc, q[0], q[1]))
            for (y, x), c in dist.items():
                iu, iv = x + u0, y + v0
                cost[self.rank[(iu >> 3, iv >> 3)]][(iu & 7) | (iv & 7) << 3] = c
            self.grids.append((u0, v0, allowed, pen))
        self._finish(cost, len(used))

    def step(self, iu, iv):
        u0, v0, allowed, pen = self.grids[self.group_of[(iu >> 3, iv >> 3)]]
        here = int(self.cost[self.where(iu, iv)])
        for k, du, dv in self.moves:
            if allowed[k][iv - v0, iu - u0]:
                c = int(self.cost[self.where(iu + du, iv + dv)])
                if c != NO_COST and c + weight(du, dv) + int(pen[iv - v0, iu - u0]) == here:
                    return k
        return 255


# ---- the second restatement ------------------------------------------------------------------------------------------
class SparseReach(_Common):
    def __init__(self, coords, cells, d2, ground_options, starts, stamp=0, **kw):
        self._setup(coords, cells, d2, ground_options, starts, stamp, kw)
        col = {}                                                        # traversable columns: (level, pen)
        for (bu, bv), r in self.rank.items():
            for w in np.flatnonzero(self.trav[r]).tolist():
                col[(8 * bu + (w & 7), 8 * bv + (w >> 3))] = (int(self.level[r, w]), int(self.pen[r, w]))
        self.col = col
        dist, queue, queued = {}, deque(), set()
        for c in self._start_columns(starts):
            if c in col and c not in dist:
                dist[c] = 0
                queue.append(c)
                queued.add(c)
        n_used = len(dist)
        while queue:
            p = queue.popleft()
            queued.discard(p)
            for k, du, dv in self.moves:
                if self.may(p, du, dv):
                    q = (p[0] + du, p[1] + dv)
                    nc = dist[p] + weight(du, dv) + col[q][1]
                    if nc < dist.get(q, 1 << 62):
                        dist[q] = nc
                        if q not in queued:
                            queue.append(q)
                            queued.add(q)
        cost = [[None] * 64 for _ in self.coords]
        for (iu, iv), c in dist.items():
            cost[self.rank[(iu >> 3, iv >> 3)]][(iu & 7) | (iv & 7) << 3] = c
        self._finish(cost, n_used)

    def may(self, p, du, dv):
        """is the move p -> p + (du, dv) allowed?"""
        need = [p, (p[0] + du, p[1] + dv)]
        if du and dv:
            need += [(p[0] + du, p[1]), (p[0], p[1] + dv)]
        if not all(q in self.col for q in need):
            return False
        levels = [self.col[q][0] for q in need]
        return max(levels) - min(levels) <= self.climb

    def step(self, iu, iv):
        here = int(self.cost[self.where(iu, iv)])
        for k, du, dv in self.moves:
            if self.may((iu, iv), du, dv):
                c = int(self.cost[self.where(iu + du, iv + dv)])
                if c != NO_COST and c + weight(du, dv) + self.col[(iu, iv)][1] == here:
                    return k
        return 255


def info_without_rounds(info):
    out = np.array(info, WORLD_GROUND_REACH_INFO).copy().reshape(1)
    out["rounds"] = 0
    return out[0]


def difference(got, want):
    """None, or what differs between two (coords, cost, info) answers - models or the library's getter; `rounds` apart"""
    for name, x, y in zip(("coords", "cost"), got[:2], want[:2]):
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape or x.dtype != y.dtype:
            return "%s: shape / dtype %s %s against %s %s" % (name, x.shape, x.dtype, y.shape, y.dtype)
        if x.tobytes() != y.tobytes():
            at = np.argwhere(x != y)
            return "%s: %d entries differ, first at %s: %s against %s" % (name, len(at), at[0], x[tuple(at[0])], y[tuple(at[0])])
    a, b = info_without_rounds(got[2]), info_without_rounds(want[2])
    if a.tobytes() != b.tobytes():
        return "info: %s against %s" % (a, b)
    return None


def answer(model):
    return model.coords, model.cost, model.info
