"""NumPy restatement of world rays (include/sdm.h: sdm_query_world_segments / sdm_query_world_views), for the tests, written
twice.

BrickWalk holds the archive as a dict from brick to its 512 words and last_stamp (what world_bricks() returns), walks a
segment with a 3-D DDA in Python floats - IEEE doubles, every crossing parameter (plane - u_a) * (1 / (u_b - u_a)) computed
fresh, x before y before z at equal t - and keeps a view's visited cells in Python sets.

DenseWalk holds a dense word grid round the case (cells beyond it, like cells of absent bricks, are unknown), finds a
segment's cells without stepping: per axis every plane whose crossing parameter is <= 1, all of them sorted by (t, axis),
applied in that order; a view's distinct counts come from np.unique over its rays' cells.

Both answer with binding.WORLD_SEGMENT_HIT / binding.VIEW_GAIN records, to be compared byte for byte.  The rays of a view
are tests/views_ref.py's (the float32 formula sdm.h pins)."""
import math

import numpy as np

from semantic_dsp_map_amd import binding
from tests import views_ref as vr

F = np.float32
UNKNOWN_WORD = 0xFF000000
CELL_LO, CELL_HI = -262144, 262144          # floor(u) of a cell whose brick is in the int16 range: [LO, HI)
MAX_CELLS = binding.WORLD_SEGMENT_MAX_CELLS

# what the discrimination checks of tests/test_world_rays_ref.py switch on, one at a time
FAULTS = ("y_before_x", "absent_is_free", "ray_sum", "truncate")


def recip_of(voxel_size):
    return F(1.0) / F(voxel_size)


def coords(p, recip):
    """u = p * recip in float32, per axis"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(p, F) * recip).astype(F)


def cell_of(u, fault=None):
    """floor(u) per axis as Python ints, or None where u is non-finite or the cell's brick lies beyond the int16 range"""
    out = []
    for v in u:
        v = float(v)
        if not math.isfinite(v):
            return None
        c = int(v) if fault == "truncate" else math.floor(v)
        if not CELL_LO <= math.floor(v) < CELL_HI:
            return None
        out.append(c)
    return out


def occ_of(word):
    o = (int(word) >> 24) & 0xFF
    return o - 256 if o >= 128 else o


def cell_class(word, ignore_movable, max_movable):
    """'occupied', 'free' or 'unknown'"""
    o = occ_of(word)
    if o == -1:
        return "unknown"
    if o >= 1 and not (ignore_movable and 1 <= (int(word) & 0xFFFF) <= max_movable):
        return "occupied"
    return "free"


def dda(ua, ub, window=None, fault=None):
    """the cells of the segment in walking order with the t at which each is entered: [(cell, t)].  window: (c0, reach) -
    the walk ends where its next step would leave it"""
    A = [float(v) for v in ua]
    D = [float(ub[i]) - A[i] for i in range(3)]
    inv = [0.0 if d == 0.0 else 1.0 / d for d in D]
    step = [1 if d > 0.0 else -1 if d < 0.0 else 0 for d in D]
    c = cell_of(ua, fault)
    tn = [math.inf if step[i] == 0 else (float(c[i] + (step[i] > 0)) - A[i]) * inv[i] for i in range(3)]
    order = (1, 0, 2) if fault == "y_before_x" else (0, 1, 2)
    t_cur, out = 0.0, []
    while True:
        out.append((tuple(c), t_cur))
        ax = order[0]
        for i in order[1:]:
            if tn[i] < tn[ax]:
                ax = i
        if tn[ax] > 1.0:
            return out
        t_cur = tn[ax]
        c[ax] += step[ax]
        tn[ax] = (float(c[ax] + (step[ax] > 0)) - A[ax]) * inv[ax]
        if window is not None and abs(c[ax] - window[0][ax]) > window[1]:
            return out


def crossings(ua, ub, window=None):
    """the same cells without stepping: every plane crossing with t <= 1, sorted by (t, axis)"""
    A = [float(v) for v in ua]
    c0 = [math.floor(a) for a in A]
    events = []
    for i in range(3):
        d = float(ub[i]) - A[i]
        if d == 0.0:
            continue
        inv, s, k = 1.0 / d, (1 if d > 0.0 else -1), 0
        while True:
            plane = c0[i] + s * k + (s > 0)
            t = (float(plane) - A[i]) * inv
            if t > 1.0 or (window is not None and k > 2 * window[1] + 1):
                break
            events.append((t, i, k, s))
            k += 1
    events.sort(key=lambda e: (e[0], e[1], e[2]))
    c, out = list(c0), [(tuple(c0), 0.0)]
    for t, i, _, s in events:
        c[i] += s
        if window is not None and abs(c[i] - window[0][i]) > window[1]:
            break
        out.append((tuple(c), t))
    return out


def span_of(ca, cb):
    return 1 + sum(abs(cb[i] - ca[i]) for i in range(3))


def no_hit(cells=0):
    h = np.zeros((), binding.WORLD_SEGMENT_HIT)
    h["t"], h["cells"], h["occ"] = -1.0, cells, -1
    return h


class _Walker:
    """what the two restatements share: the rules round a walk.  A subclass gives lookup(cell) -> (word, stamp) and
    cells_of(ua, ub, window)."""
    fault = None

    def lookup(self, cell):
        raise NotImplementedError

    def cells_of(self, ua, ub, window):
        raise NotImplementedError

    def walk(self, ua, ub, unknown_blocks, ignore_movable, window=None):
        """-> (hit record, [(cell, class)] of the visited cells, the blocking one included)"""
        visited, unknown = [], 0
        h = no_hit()
        for cell, t in self.cells_of(ua, ub, window):
            word, stamp = self.lookup(cell)
            cls = cell_class(word, ignore_movable, self.max_movable)
            blocks = cls == "occupied" or (unknown_blocks and cls == "unknown")
            visited.append((cell, cls))
            unknown += cls == "unknown"
            if blocks:
                h["t"], h["cell"], h["stamp"] = F(t), cell, stamp
                h["track"], h["label"], h["occ"] = int(word) & 0xFFFF, (int(word) >> 16) & 0xFF, occ_of(word)
                break
        h["cells"], h["unknown"] = len(visited), unknown
        return h, visited

    def segments(self, a, b, unknown_blocks=False, ignore_movable=False):
        a, b = np.asarray(a, F).reshape(-1, 3), np.asarray(b, F).reshape(-1, 3)
        out = np.zeros(len(a), binding.WORLD_SEGMENT_HIT)
        for i in range(len(a)):
            ua, ub = coords(a[i], self.recip), coords(b[i], self.recip)
            ca, cb = cell_of(ua), cell_of(ub)
            if ca is None or cb is None:               # invalid
                out[i] = no_hit()
                if unknown_blocks:
                    out[i]["t"] = 0.0
            elif span_of(ca, cb) > MAX_CELLS:          # too long
                out[i] = no_hit(-1)
            else:
                out[i] = self.walk(ua, ub, unknown_blocks, ignore_movable)[0]
        return out

    def views(self, views, dirs, reach, ignore_movable=False):
        """-> (gain [n_views], rays [n_views, n_rays])"""
        views = np.asarray(views, binding.VIEW).reshape(-1)
        a, b, given = vr.rays_of(views, dirs)
        nv, nr = given.shape
        gain, rays = np.zeros(nv, binding.VIEW_GAIN), np.zeros((nv, nr), binding.WORLD_SEGMENT_HIT)
        for v in range(nv):
            rays[v] = no_hit()
            ua = coords(views["pos"][v], self.recip)
            c0 = cell_of(ua)
            view_ok = (np.isfinite(views["pos"][v]).all() and np.isfinite(views["q"][v]).all() and np.isfinite(views["range"][v]) and c0 is not None
                       and all(CELL_LO <= c - reach and c + reach < CELL_HI for c in c0))
            if not view_ok:
                continue
            seen = []
            for r in range(nr):
                ub = coords(b[v, r], self.recip)
                if not given[v, r] or not np.isfinite(ub).all():
                    continue
                rays[v, r], visited = self.walk(ua, ub, False, ignore_movable, window=(c0, reach))
                seen.extend(visited)
            g = gain[v]
            g["rays_hit"] = int((rays[v]["t"] >= 0).sum())
            g["rays_in_map"] = int((rays[v]["cells"] > 0).sum())
            g["ray_cells"], g["ray_unknown"] = int(rays[v]["cells"].sum()), int(rays[v]["unknown"].sum())
            for cls, n in self.distinct(seen).items():
                g["n_" + cls] = n
        return gain, rays

    def distinct(self, seen):
        raise NotImplementedError


class BrickWalk(_Walker):
    """the archive as a dict of bricks; the DDA in Python floats; the masks as Python sets"""

    def __init__(self, hdr, cells, voxel_size, max_movable, fault=None):
        self.recip, self.max_movable, self.fault = recip_of(voxel_size), int(max_movable), fault
        self.bricks = {(int(h["bx"]), int(h["by"]), int(h["bz"])): (np.asarray(cells[i], np.uint32), int(h["last_stamp"])) for i, h in enumerate(hdr)}

    def lookup(self, cell):
        b = (cell[0] >> 3, cell[1] >> 3, cell[2] >> 3)
        if not all(-32768 <= v <= 32767 for v in b) or b not in self.bricks:
            return (0 if self.fault == "absent_is_free" else UNKNOWN_WORD), 0
        words, stamp = self.bricks[b]
        return int(words[(cell[0] & 7) | (cell[1] & 7) << 3 | (cell[2] & 7) << 6]), stamp

    def cells_of(self, ua, ub, window):
        return dda(ua, ub, window, self.fault)

    def distinct(self, seen):
        if self.fault == "ray_sum":
            return {cls: sum(1 for _, k in seen if k == cls) for cls in ("unknown", "free", "occupied")}
        sets = {"unknown": set(), "free": set(), "occupied": set()}
        for cell, cls in seen:
            sets[cls].add(cell)
        return {cls: len(s) for cls, s in sets.items()}


class DenseWalk(_Walker):
    """a dense word grid and a dense stamp grid [z, y, x] over the bricks' bounding box; the cells of a segment from its
    sorted plane crossings; distinct counts with np.unique"""

    def __init__(self, hdr, cells, voxel_size, max_movable):
        self.recip, self.max_movable = recip_of(voxel_size), int(max_movable)
        b = np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int64).reshape(-1, 3)
        self.lo = b.min(axis=0) * 8 if len(b) else np.zeros(3, np.int64)
        size = (b.max(axis=0) - b.min(axis=0) + 1) * 8 if len(b) else np.zeros(3, np.int64)
        self.words = np.full(tuple(size[::-1]), UNKNOWN_WORD, np.uint32)
        self.stamps = np.zeros(tuple(size[::-1]), np.uint32)
        for i in range(len(b)):
            x, y, z = b[i] * 8 - self.lo
            self.words[z:z + 8, y:y + 8, x:x + 8] = np.asarray(cells[i], np.uint32).reshape(8, 8, 8)
            self.stamps[z:z + 8, y:y + 8, x:x + 8] = hdr["last_stamp"][i]

    def lookup(self, cell):
        r = np.asarray(cell, np.int64) - self.lo
        if (r < 0).any() or (r >= np.array(self.words.shape[::-1])).any():
            return UNKNOWN_WORD, 0
        return int(self.words[r[2], r[1], r[0]]), int(self.stamps[r[2], r[1], r[0]])

    def cells_of(self, ua, ub, window):
        return crossings(ua, ub, window)

    def distinct(self, seen):
        out = {}
        for cls in ("unknown", "free", "occupied"):
            c = np.array([cell for cell, k in seen if k == cls], np.int64).reshape(-1, 3)
            out[cls] = len(np.unique(c, axis=0))
        return out
