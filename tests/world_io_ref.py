"""NumPy restatement of the world archive's import and retain (include/sdm.h: sdm_world_import / sdm_world_retain), on top
of tests/world_ref.py, for the tests.

Written twice, as world_ref.py is.  `Archive` (world_ref.Archive with an import count) with import_bricks() and retain()
is the brick model: sources deduplicated by lowest index, the destinations enumerated and taken in brick order, the
incoming 512 words of each gathered from its up to 8 sources, ranked under the capacity rule, stamps by min / max over the
contributors.  `Naive` (world_ref.Naive with a stamp pair per brick) with import_cells() and retain() goes cell by cell:
world cell of the source plus the offset, nothing else; tests/test_world_io_ref.py holds the first against the second."""
import itertools

import numpy as np

from semantic_dsp_map_amd import binding
from tests import world_ref as wr

UNKNOWN = wr.UNKNOWN
MAX_OFFSET = 1 << 19
_W = np.arange(512)
_C = np.stack([_W & 7, (_W >> 3) & 7, _W >> 6], 1)                   # cell (x, y, z) of every cell word


def coords(hdr):
    return [(int(h["bx"]), int(h["by"]), int(h["bz"])) for h in hdr]


def in_range(b):
    return all(wr.B_MIN <= int(v) <= wr.B_MAX for v in b)


def make_headers(coord, first=1, last=1):
    """WORLD_BRICK headers of bricks at `coord` (n, 3); the counts are left 0: an import takes them again"""
    coord = np.asarray(coord, np.int64).reshape(-1, 3)
    hdr = np.zeros(len(coord), binding.WORLD_BRICK)
    hdr["bx"], hdr["by"], hdr["bz"] = coord[:, 0], coord[:, 1], coord[:, 2]
    hdr["first_stamp"], hdr["last_stamp"] = first, last
    return hdr


class Archive(wr.Archive):
    """world_ref.Archive, valid after an import as well: n_updates, flags and stamp keep describing the last update"""

    def __init__(self, max_bricks):
        super().__init__(max_bricks)
        self.n_imports = 0

    def info(self):
        if self.n_updates or not self.n_imports:
            return super().info()
        self.n_updates = 1
        try:
            out = super().info()
        finally:
            self.n_updates = 0
        out["n_updates"] = 0
        return out


def first_of_each(hdr):
    """brick -> the lowest source index with these coordinates"""
    src = {}
    for i, key in enumerate(coords(hdr)):
        src.setdefault(key, i)
    return src


def import_bricks(A, hdr, cells, offset=(0, 0, 0), max_movable=0, flags=0, fill=False):
    """one sdm_world_import on the brick model; flags: STATIC_ONLY | OBSERVED_ONLY"""
    hdr, cells = np.asarray(hdr), np.asarray(cells, np.uint32).reshape(-1, 512)
    off = np.asarray(offset, np.int64)
    assert (np.abs(off) <= MAX_OFFSET).all()
    if not len(hdr):
        return A
    q, r = off >> 3, off & 7
    src = first_of_each(hdr)
    steps = [(0, 1) if r[a] else (0,) for a in range(3)]
    dest = {tuple(int(v) for v in np.array(key) + q + e) for key in src for e in itertools.product(*steps)}
    # per destination cell: which of the 8 sources it comes from (c < r per axis) and which cell of it ((c - r) & 7)
    up = (_C < r).astype(np.int64)
    from_cell = (_C - r) & 7
    from_word = from_cell[:, 0] | (from_cell[:, 1] << 3) | (from_cell[:, 2] << 6)
    created = dropped = out_of_range = 0
    n_before = len(A.coord)
    for d in sorted(dest, key=lambda b: (b[2], b[1], b[0])):
        inc, who = np.full(512, UNKNOWN, np.uint32), np.full(512, -1, np.int64)
        for e in itertools.product((0, 1), repeat=3):
            i = src.get(tuple(int(v) for v in np.array(d) - q - e))
            if i is not None:
                m = (up == e).all(axis=1)
                inc[m], who[m] = cells[i][from_word[m]], i
        s = A.slot.get(d)
        mask = wr.writes(inc, max_movable, flags)
        if fill and s is not None:
            mask &= wr.occ_of(A.cells[s]) < 0
        if not mask.any():
            continue
        if not in_range(d):
            out_of_range += 1
            continue
        gave = np.unique(who[mask])
        first, last = int(hdr["first_stamp"][gave].min()), int(hdr["last_stamp"][gave].max())
        if s is None:
            if n_before + created >= A.max_bricks:
                dropped += int(mask.sum())
                continue
            s = n_before + created
            created += 1
            A.slot[d] = s
            A.coord.append(d)
            A.first_stamp.append(first)
            A.last_stamp.append(last)
            A.cells.append(np.full(512, UNKNOWN, np.uint32))
        else:
            A.first_stamp[s], A.last_stamp[s] = min(A.first_stamp[s], first), max(A.last_stamp[s], last)
        A.cells[s][mask] = inc[mask]
    A.n_imports += 1
    A.created_last, A.dropped_last, A.out_of_range_last = created, dropped, out_of_range
    A.dropped_total += dropped
    return A


def keeps(coord, last_stamp, bmin, bmax, min_last_stamp):
    lo = (wr.B_MIN,) * 3 if bmin is None else bmin
    hi = (wr.B_MAX,) * 3 if bmax is None else bmax
    return all(int(lo[a]) <= coord[a] <= int(hi[a]) for a in range(3)) and int(last_stamp) >= int(min_last_stamp)


def retain(A, bmin=None, bmax=None, min_last_stamp=0):
    """one sdm_world_retain on the brick model -> the number of bricks removed"""
    keep = [s for s in range(len(A.coord)) if keeps(A.coord[s], A.last_stamp[s], bmin, bmax, min_last_stamp)]
    removed = len(A.coord) - len(keep)
    A.coord = [A.coord[s] for s in keep]
    A.cells = [A.cells[s] for s in keep]
    A.first_stamp = [A.first_stamp[s] for s in keep]
    A.last_stamp = [A.last_stamp[s] for s in keep]
    A.slot = {c: k for k, c in enumerate(A.coord)}
    return removed


# ---- the naive model: world cell -> word, brick -> [first_stamp, last_stamp]
class Naive(wr.Naive):
    def __init__(self):
        super().__init__()
        self.stamps = {}

    def import_cells(self, hdr, cells, offset=(0, 0, 0), max_movable=0, flags=0, fill=False, skip_bricks=()):
        """every writing cell of the first source of each brick lands on its world cell plus the offset; skip_bricks: the
        destination bricks the capacity rule left out of this import"""
        cells = np.asarray(cells, np.uint32).reshape(-1, 512)
        skip, seen, new = set(skip_bricks), set(), {}
        off = [int(v) for v in offset]
        for i, key in enumerate(coords(hdr)):
            if key in seen:
                continue
            seen.add(key)
            wrote = wr.writes(cells[i], max_movable, flags)
            for w in np.nonzero(wrote)[0].tolist():
                g = tuple(8 * key[a] + ((w >> (3 * a)) & 7) + off[a] for a in range(3))
                b = tuple(v >> 3 for v in g)
                if b in skip or not in_range(b):
                    continue
                if fill and (self.cell.get(g, UNKNOWN) >> 24) < 128:
                    continue
                new[g] = int(cells[i][w])
                st = self.stamps.setdefault(b, [int(hdr["first_stamp"][i]), int(hdr["last_stamp"][i])])
                st[0], st[1] = min(st[0], int(hdr["first_stamp"][i])), max(st[1], int(hdr["last_stamp"][i]))
        self.cell.update(new)

    def retain(self, bmin=None, bmax=None, min_last_stamp=0):
        gone = {b for b, st in self.stamps.items() if not keeps(b, st[1], bmin, bmax, min_last_stamp)}
        self.cell = {g: w for g, w in self.cell.items() if tuple(v >> 3 for v in g) not in gone}
        for b in gone:
            del self.stamps[b]
        return len(gone)
