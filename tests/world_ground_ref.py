"""NumPy restatement of the world ground layer (include/sdm.h: sdm_world_ground_update / sdm_get_world_ground /
sdm_query_world_ground / sdm_query_world_footprints), for the tests.  No SciPy.  Written twice:

  * DenseModel: per tile a dense grid of archived words in WORLD coordinates (x, y, z) - the tile's columns and a margin of
    R + 1 columns, the read window along the up axis -, filled brick by brick, unknown where the archive has nothing; turned
    to (height, v, u) by a transpose and a flip; the columns by one walk from the window's top down that carries the run of
    passable cells; the step bit on the dense level grid; the distance by brute force over the lethal columns of the margin.
    A tile exists where a brick's own heights 8 hb .. 8 hb + 7 meet the window.
  * ColumnModel: the bricks once as (height brick, bv, bu) -> [hl, cv, cu]; per tile the window's cells as one array
    [rel, 64] put together from its bricks; no walk: "the first blocked cell above" by a reversed running minimum, supports,
    level, top and headroom from it; the step bit through a dictionary of the tiles' levels; the distance by the two
    truncated passes (rows, then columns) over the lethal bits of the (2 H + 1)^2 tiles round the tile.  A tile exists where
    a brick's height-brick index lies between the window's.

Both take what a caller can read back - world_bricks() - and give coords, cells, d2 and the info block;
tests/test_world_ground_ref.py holds one to the other, tests/test_world_ground_gpu.py the library to ColumnModel.  The two
queries are restated once, on a model's answer.  World cells are (x, y, z); a brick's cell word is cx | cy << 3 | cz << 6; a
tile's column word is cu | cv << 3."""
import numpy as np

from semantic_dsp_map_amd.binding import (FOOTPRINT, GROUND_CELL, WORLD_FOOTPRINT_RESULT, WORLD_GROUND_ABSENT_IS_LETHAL, WORLD_GROUND_BOX,
                                          WORLD_GROUND_FAR, WORLD_GROUND_IGNORE_MOVABLE, WORLD_GROUND_INFO, WORLD_GROUND_NONE,
                                          WORLD_GROUND_NONE_IS_LETHAL, WORLD_GROUND_OPTIONS, WORLD_GROUND_RESULT,
                                          WORLD_GROUND_UNKNOWN_PASSABLE, label_mask)

B_MIN, B_MAX = -32768, 32767
C_MIN, C_MAX = -262144, 262143
NO = 0xFFFF
UNKNOWN = 0xFF000000
INT32_MIN = -(1 << 31)


def options_of(up=(2, 1), h_lo=0, h_hi=0, clearance=0, max_step=0, radius=8, support_labels=None, unknown_passable=False, ignore_movable=False,
               none_is_lethal=False, absent_is_lethal=False, box=None):
    """the WORLD_GROUND_OPTIONS record SdmMap.world_ground_update hands to the library"""
    o = np.zeros(1, WORLD_GROUND_OPTIONS)[0]
    o["up_axis"], o["up_sign"] = up
    o["h_lo"], o["h_hi"], o["clearance"], o["max_step"], o["radius"] = h_lo, h_hi, clearance, max_step, radius
    o["support_labels"] = label_mask(support_labels)
    o["flags"] = ((WORLD_GROUND_UNKNOWN_PASSABLE if unknown_passable else 0) | (WORLD_GROUND_IGNORE_MOVABLE if ignore_movable else 0) |
                  (WORLD_GROUND_NONE_IS_LETHAL if none_is_lethal else 0) | (WORLD_GROUND_ABSENT_IS_LETHAL if absent_is_lethal else 0) |
                  (WORLD_GROUND_BOX if box is not None else 0))
    if box is not None:
        o["tmin"], o["tmax"] = box[0], box[1]
    return o


def classes(words, o, max_movable):
    """solid, blocked (not passable), candidate, unknown and the label of archived words, any shape"""
    w = np.asarray(words, np.uint32)
    flags = int(o["flags"])
    occ = ((w >> 24) & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64)
    track, label = (w & 0xFFFF).astype(np.int64), ((w >> 16) & 0xFF).astype(np.int64)
    movable = (track >= 1) & (track <= max_movable)
    solid = (occ >= 1) & ~(movable & bool(flags & WORLD_GROUND_IGNORE_MOVABLE))
    passable = (occ == 0) | ((occ >= 1) & ~solid) | ((occ == -1) & bool(flags & WORLD_GROUND_UNKNOWN_PASSABLE))
    in_mask = ((np.asarray(o["support_labels"], np.uint32)[label >> 5] >> (label & 31).astype(np.uint32)) & 1).astype(bool)
    return solid, ~passable, solid & ~movable & in_mask, occ == -1, label


def axes_of(o):
    a = int(o["up_axis"])
    return a, (1 if a == 0 else 0), (1 if a == 2 else 2)


def in_box(o, bu, bv):
    if not int(o["flags"]) & WORLD_GROUND_BOX:
        return True
    return int(o["tmin"][0]) <= bu <= int(o["tmax"][0]) and int(o["tmin"][1]) <= bv <= int(o["tmax"][1])


class _Common:
    def _finish(self, o, tiles, cells, d2, stamp):
        """tiles: (bu, bv) in order; cells: per tile a dict of int arrays [64] level, top, label, cls, headroom, n_unknown"""
        n = len(tiles)
        self.o = o
        self.coords = np.asarray(tiles, np.int64).reshape(-1, 2).astype(np.int16)
        self.cells = np.zeros((n, 64), GROUND_CELL)
        for r, c in enumerate(cells):
            for f in GROUND_CELL.names:
                self.cells[f][r] = c[f]
        R = int(o["radius"])
        d2 = np.asarray(d2, np.int64).reshape(n, 64)
        self.d2 = np.where(d2 > R * R, WORLD_GROUND_NONE, d2).astype(np.uint16)
        k = self.cells["cls"] & 3
        self.info = np.zeros(1, WORLD_GROUND_INFO)[0]
        self.info["n_tiles"], self.info["stamp"], self.info["options"] = n, stamp, o
        self.info["n_ground"], self.info["n_obstacle"], self.info["n_none"] = (k == 1).sum(), (k == 2).sum(), (k == 0).sum()
        self.info["n_step"], self.info["n_lethal"] = ((self.cells["cls"] >> 2) & 1).sum(), ((self.cells["cls"] >> 3) & 1).sum()
        lv = self.cells["level"][k == 1]
        self.info["level_min"], self.info["level_max"] = (lv.min(), lv.max()) if len(lv) else (NO, NO)
        self.rank = {tuple(t): r for r, t in enumerate(self.coords.astype(np.int64).tolist())}

    def query(self, cells, voxel_size):
        """WORLD_GROUND_RESULT per world cell of `cells` (n, 3)"""
        o = self.o
        a, au, av = axes_of(o)
        sign, h_lo, R = int(o["up_sign"]), int(o["h_lo"]), int(o["radius"])
        size = np.float32(voxel_size)
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        out = np.zeros(len(cells), WORLD_GROUND_RESULT)
        out["d2"], out["above"], out["dist"], out["status"] = 0xFFFFFFFF, INT32_MIN, -1.0, 3
        out["cell"]["level"] = out["cell"]["top"] = NO
        for i, g in enumerate(cells.tolist()):
            if not all(C_MIN <= v <= C_MAX for v in g):
                continue
            iu, iv = g[au], g[av]
            out[i]["col"] = (iu, iv)
            r = self.rank.get((iu >> 3, iv >> 3))
            if r is None:
                continue
            w = (iu & 7) | (iv & 7) << 3
            c, v = self.cells[r, w], int(self.d2[r, w])
            out[i]["cell"], out[i]["status"] = c, 0
            if v == WORLD_GROUND_NONE:
                out[i]["d2"], out[i]["dist"] = WORLD_GROUND_FAR, np.sqrt(np.float32(R * R + 1)) * size
            else:
                out[i]["d2"], out[i]["dist"] = v, np.sqrt(np.float32(v)) * size
            if c["level"] != NO:
                hl = h_lo + int(c["level"])
                out[i]["above"] = (g[a] if sign > 0 else -1 - g[a]) - hl
                out[i]["surface"] = np.float32(hl + 1 if sign > 0 else -1 - hl) * size
        return out

    def footprints(self, fps, voxel_size):
        """WORLD_FOOTPRINT_RESULT per FOOTPRINT record: every column of a square that holds whatever the rule can cover"""
        size = np.float32(voxel_size)
        fps = np.asarray(fps, FOOTPRINT).reshape(-1)
        out = np.zeros(len(fps), WORLD_FOOTPRINT_RESULT)
        out["level_min"] = out["level_max"] = NO
        out["min_d2"] = 0xFFFFFFFF
        f32 = np.float32
        for k, fp in enumerate(fps):
            v = [f32(fp[f]) for f in FOOTPRINT.names]
            cu, cv, du_, dv_, hl, hw = v
            with np.errstate(all="ignore"):
                reach = f32(hl + hw)
                if not np.isfinite(np.array(v)).all() or reach > f32(64) * size or f32(f32(du_ * du_) + f32(dv_ * dv_)) < f32(0.5):
                    continue
            m = 2 * 64 + 8                         # columns: sqrt(2) * 64 and then some
            iu0, iv0 = int(np.floor(float(cu) / float(size))), int(np.floor(float(cv) / float(size)))
            i = np.arange(max(iu0 - m, C_MIN), min(iu0 + m, C_MAX) + 1, dtype=np.int64)
            j = np.arange(max(iv0 - m, C_MIN), min(iv0 + m, C_MAX) + 1, dtype=np.int64)
            if not len(i) or not len(j):
                continue
            pu = ((i.astype(f32) + f32(0.5)) * size)[None, :]
            pv = ((j.astype(f32) + f32(0.5)) * size)[:, None]
            du, dv = (pu - cu).astype(f32), (pv - cv).astype(f32)
            along = np.abs(((du * du_).astype(f32) + (dv * dv_).astype(f32)).astype(f32))
            across = np.abs(((dv * du_).astype(f32) - (du * dv_).astype(f32)).astype(f32))
            cov = np.argwhere((along <= hl) & (across <= hw))       # (row j, column i): ascending in (v, u)
            first = None
            lv = []
            for jj, ii in cov.tolist():
                iu, iv = int(i[ii]), int(j[jj])
                r = self.rank.get((iu >> 3, iv >> 3))
                if r is None:
                    out[k]["n_absent"] += 1
                    continue
                w = (iu & 7) | (iv & 7) << 3
                c, d = self.cells[r, w], int(self.d2[r, w])
                out[k]["n_cols"] += 1
                out[k]["min_d2"] = min(int(out[k]["min_d2"]), WORLD_GROUND_FAR if d == WORLD_GROUND_NONE else d)
                if c["cls"] & 8:
                    out[k]["n_lethal"] += 1
                    first = first or (iu, iv)
                    if first == (iu, iv):
                        out[k]["first_lethal"] = first
                if c["cls"] & 3 == 1:
                    out[k]["n_ground"] += 1
                    lv.append(int(c["level"]))
                out[k]["n_none"] += int(c["cls"] & 3 == 0)
            if lv:
                out[k]["level_min"], out[k]["level_max"] = min(lv), max(lv)
        return out


def brick_dict(hdr, cells):
    coord = np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int64).reshape(-1, 3)
    words = np.asarray(cells, np.uint32).reshape(-1, 8, 8, 8)       # [j, cz, cy, cx]
    return {tuple(b): words[j] for j, b in enumerate(coord.tolist())}


def sorted_tiles(tiles):
    return sorted(tiles, key=lambda t: (t[1], t[0]))


# ---- the first restatement ---------------------------------------------------------------------------------------------
class DenseModel(_Common):
    def __init__(self, hdr, cells, max_movable, stamp=0, **kw):
        o = options_of(**kw)
        a, au, av = axes_of(o)
        sign, h_lo, h_hi, clr = int(o["up_sign"]), int(o["h_lo"]), int(o["h_hi"]), int(o["clearance"])
        R, max_step, flags = int(o["radius"]), int(o["max_step"]), int(o["flags"])
        h_top, M = h_hi + clr, R + 1
        bricks = brick_dict(hdr, cells)
        tiles = set()
        for b in bricks:
            lo = 8 * b[a] if sign > 0 else -1 - (8 * b[a] + 7)     # the brick's own heights lo .. lo + 7
            if lo <= h_top and lo + 7 >= h_lo and in_box(o, b[au], b[av]):
                tiles.add((b[au], b[av]))
        tiles = sorted_tiles(tiles)
        tset = set(tiles)
        g0, g1 = (h_lo, h_top) if sign > 0 else (-1 - h_top, -1 - h_lo)    # the window as coordinates of the up axis
        nh, nc = h_top - h_lo + 1, 8 + 2 * M
        out_cells, out_d2 = [], []
        for bu, bv in tiles:
            lo = [0, 0, 0]
            lo[a], lo[au], lo[av] = g0, 8 * bu - M, 8 * bv - M
            n = [0, 0, 0]
            n[a], n[au], n[av] = nh, nc, nc
            grid = np.full((n[2], n[1], n[0]), UNKNOWN, np.uint32)      # [z, y, x]
            rng = [range(lo[k] >> 3, ((lo[k] + n[k] - 1) >> 3) + 1) for k in range(3)]
            for bz in rng[2]:
                for by in rng[1]:
                    for bx in rng[0]:
                        q = (bx, by, bz)
                        src = bricks.get(q) if all(B_MIN <= v <= B_MAX for v in q) else None
                        if src is None:
                            continue
                        at = [8 * q[k] - lo[k] for k in range(3)]
                        s = [slice(max(v, 0), min(v + 8, n[k])) for k, v in enumerate(at)]
                        c = [slice(sl.start - v, sl.stop - v) for sl, v in zip(s, at)]
                        grid[s[2], s[1], s[0]] = src[c[2], c[1], c[0]]
            H = grid.transpose(2 - a, 2 - av, 2 - au)                   # [g, v, u]
            if sign < 0:
                H = H[::-1]                                             # [rel, v, u]
            ui, vi = np.arange(nc) + lo[au], np.arange(nc) + lo[av]
            exists = np.array([[(int(u) >> 3, int(v) >> 3) in tset for u in ui] for v in vi])
            solid, blocked, cand, unknown, label = classes(H, o, max_movable)
            shape = (nc, nc)
            level, top = np.full(shape, NO, np.int64), np.full(shape, NO, np.int64)
            lab, head, n_unk, run = (np.zeros(shape, np.int64) for _ in range(4))
            for rel in range(nh - 1, -1, -1):                           # from the window's top down
                if rel <= h_hi - h_lo:
                    top = np.where(solid[rel] & (top == NO), rel, top)
                    take = cand[rel] & (level == NO) & (run >= clr)
                    level, lab, head = np.where(take, rel, level), np.where(take, label[rel], lab), np.where(take, run, head)
                    n_unk = n_unk + unknown[rel]
                run = np.where(blocked[rel], 0, run + 1)
            cls = np.where(level != NO, 1, np.where(top != NO, 2, 0))
            has = exists & (level != NO)
            step = np.zeros(shape, bool)
            inner = (slice(1, -1), slice(1, -1))
            for dv, du in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                q = (slice(1 + dv, nc - 1 + dv), slice(1 + du, nc - 1 + du))
                step[inner] |= has[inner] & has[q] & (level[inner] > level[q] + max_step)
            lethal = np.where(exists, (cls == 2) | step | ((cls == 0) & bool(flags & WORLD_GROUND_NONE_IS_LETHAL)),
                              bool(flags & WORLD_GROUND_ABSENT_IS_LETHAL))
            lethal[0, :] = lethal[-1, :] = lethal[:, 0] = lethal[:, -1] = False   # (the outermost ring has no step bit: beyond R anyway)
            lv, lu = np.nonzero(lethal)
            own = (slice(M, M + 8), slice(M, M + 8))
            d2 = np.full((8, 8), 1 << 20, np.int64)
            for cv in range(8):
                for cu in range(8):
                    if len(lv):
                        d2[cv, cu] = ((lv - (M + cv)) ** 2 + (lu - (M + cu)) ** 2).min()
            out_cells.append(dict(level=level[own].reshape(64), top=top[own].reshape(64), label=lab[own].reshape(64),
                                  cls=(cls | step.astype(np.int64) << 2 | lethal.astype(np.int64) << 3)[own].reshape(64), headroom=np.minimum(head[own], 255).reshape(64),
                                  n_unknown=np.minimum(n_unk[own], 255).reshape(64)))
            out_d2.append(d2.reshape(64))
        self._finish(o, tiles, out_cells, out_d2, stamp)


# ---- the second restatement ------------------------------------------------------------------------------------------
class ColumnModel(_Common):
    def __init__(self, hdr, cells, max_movable, stamp=0, **kw):
        o = options_of(**kw)
        a, au, av = axes_of(o)
        sign, h_lo, h_hi, clr = int(o["up_sign"]), int(o["h_lo"]), int(o["h_hi"]), int(o["clearance"])
        R, max_step, flags = int(o["radius"]), int(o["max_step"]), int(o["flags"])
        span, rel_top = h_hi - h_lo, h_hi - h_lo + clr
        hb_lo, hb_top = h_lo >> 3, (h_lo + rel_top) >> 3
        canon = {}                                                      # (hb, bv, bu) -> [hl, cv, cu]
        for b, w in brick_dict(hdr, cells).items():
            c = w.transpose(2 - a, 2 - av, 2 - au)
            canon[(b[a], b[av], b[au]) if sign > 0 else (-1 - b[a], b[av], b[au])] = c if sign > 0 else c[::-1]
        tiles = sorted_tiles({(bu, bv) for hb, bv, bu in canon if hb_lo <= hb <= hb_top and in_box(o, bu, bv)})
        col = {}
        for bu, bv in tiles:
            parts = []
            for hb in range(hb_lo, hb_top + 1):
                ba = hb if sign > 0 else -1 - hb
                src = canon.get((hb, bv, bu)) if B_MIN <= ba <= B_MAX else None
                parts.append(np.full((8, 64), UNKNOWN, np.uint32) if src is None else src.reshape(8, 64))
            first = h_lo - 8 * hb_lo
            win = np.concatenate(parts)[first:first + rel_top + 1]      # [rel, column]
            solid, blocked, cand, unknown, label = classes(win, o, max_movable)
            nh = rel_top + 1
            idx = np.arange(nh)[:, None]
            # the first blocked cell at or above each height, then strictly above: nh where there is none inside the window
            at_or_above = np.minimum.accumulate(np.where(blocked, idx, nh)[::-1], axis=0)[::-1]
            above = np.concatenate([at_or_above[1:], np.full((1, 64), nh)])
            room = above - idx - 1                                      # passable cells directly above, inside the window
            band = idx <= span
            support = cand & band & (room >= clr)
            level = np.where(support.any(axis=0), nh - 1 - np.argmax(support[::-1], axis=0), NO)
            sb = solid & band
            top = np.where(sb.any(axis=0), nh - 1 - np.argmax(sb[::-1], axis=0), NO)
            at = np.where(level == NO, 0, level)
            cols = np.arange(64)
            col[(bu, bv)] = dict(level=level, top=top, label=np.where(level == NO, 0, label[at, cols]),
                                 headroom=np.where(level == NO, 0, np.minimum(room[at, cols], 255)),
                                 n_unknown=np.minimum((unknown & band).sum(axis=0), 255))
        for (bu, bv), c in col.items():
            lv = c["level"].reshape(8, 8)                               # [cv, cu]
            ring = np.full((10, 10), NO, np.int64)
            ring[1:9, 1:9] = lv
            for (du, dv), dst, src in (((-1, 0), (slice(1, 9), 0), (slice(None), 7)), ((1, 0), (slice(1, 9), 9), (slice(None), 0)),
                                       ((0, -1), (0, slice(1, 9)), (7, slice(None))), ((0, 1), (9, slice(1, 9)), (0, slice(None)))):
                q = col.get((bu + du, bv + dv))
                if q is not None:
                    ring[dst] = q["level"].reshape(8, 8)[src]
            step = np.zeros((8, 8), bool)
            for sl in ((slice(1, 9), slice(0, 8)), (slice(1, 9), slice(2, 10)), (slice(0, 8), slice(1, 9)), (slice(2, 10), slice(1, 9))):
                step |= (lv != NO) & (ring[sl] != NO) & (lv > ring[sl] + max_step)
            k = np.where(c["level"] != NO, 1, np.where(c["top"] != NO, 2, 0))
            step = step.reshape(64)
            lethal = (k == 2) | step | ((k == 0) & bool(flags & WORLD_GROUND_NONE_IS_LETHAL))
            c["cls"], c["lethal"] = k | step.astype(np.int64) << 2 | lethal.astype(np.int64) << 3, lethal.reshape(8, 8)
        H = 1 if R <= 8 else 2
        S = 8 * (2 * H + 1)
        out_d2 = []
        for bu, bv in tiles:
            area = np.full((S, S), bool(flags & WORLD_GROUND_ABSENT_IS_LETHAL))    # [v, u]
            for ov in range(-H, H + 1):
                for ou in range(-H, H + 1):
                    q = col.get((bu + ou, bv + ov))
                    if q is not None:
                        area[8 * (ov + H):8 * (ov + H) + 8, 8 * (ou + H):8 * (ou + H) + 8] = q["lethal"]
            rows = np.full((S, 8), 1 << 10, np.int64)                   # along u, per column of the tile
            for t in range(R, -1, -1):
                for s_ in (-1, 1):
                    shifted = area[:, 8 * H + s_ * t:8 * H + s_ * t + 8]
                    rows = np.where(shifted, t, rows)
            d2 = np.full((8, 8), 1 << 20, np.int64)
            for k in range(-R, R + 1):
                part = rows[8 * H + k:8 * H + k + 8]
                v = part * part + k * k
                d2 = np.where((v <= R * R) & (v < d2), v, d2)
            out_d2.append(d2.reshape(64))
        self._finish(o, tiles, [col[t] for t in tiles], out_d2, stamp)


def difference(got, want):
    """None, or what differs between two (coords, cells, d2, info) answers - models or the library's getter"""
    for name, x, y in zip(("coords", "cells", "d2", "info"), got, want):
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape or x.dtype != y.dtype:
            return "%s: shape / dtype %s %s against %s %s" % (name, x.shape, x.dtype, y.shape, y.dtype)
        if x.tobytes() != y.tobytes():
            if x.dtype.names:
                bad = [f for f in x.dtype.names if x[f].tobytes() != y[f].tobytes()]
                at = np.argwhere(np.asarray(x[bad[0]] != y[bad[0]]).reshape(x.shape + (-1,)).any(axis=-1)) if x.shape else []
                where = " first at %s" % (at[0],) if len(at) else ""
                pick = (lambda v: v[tuple(at[0])]) if len(at) else (lambda v: v)
                return "%s: fields %s differ:%s %s against %s" % (name, bad, where, pick(x[bad[0]]), pick(y[bad[0]]))
            at = np.argwhere(x != y)
            return "%s: %d entries differ, first at %s: %s against %s" % (name, len(at), at[0], x[tuple(at[0])], y[tuple(at[0])])
    return None


def answer(model):
    return model.coords, model.cells, model.d2, model.info
