"""NumPy / Python restatement of the world changes (include/sdm.h: sdm_world_changes_update / sdm_get_world_changes /
sdm_get_world_change_cells / sdm_get_world_change_labels / sdm_query_world_changes), for the tests.  No SciPy.  Written twice:

  * BrickModel: the block laid over the bricks it overlaps (world_ref.brick_view: the candidates in brick order, 512 words
    each in cell-word order) against the archived brick of each candidate; per candidate the listed cells as eight 64-bit
    layer words (bit cx + 8 cy); the cell list is the listed words' bits in order, a cell's list index its word's prefix
    plus the set bits below its own; the regions are a union-find over list indices whose root is the smallest index.
  * CellModel: a dense grid of world cells over the candidates' box, one (now, before) pair per cell, the archive side filled
    in brick by brick; the listed cells go into a dict from world cell to list index and a breadth-first search in list
    order steps only to listed cells of an equal key.

Both take what a caller can read back - the block's word grid [z, y, x] (esdf_ref.snapshot_grid of voxels()) with the
ring's moved_steps and stamp, and world_bricks() with the archive's stamp - and give the cell list, the region index per
cell, the table, the per-label counters and the info record; tests/test_world_changes_ref.py holds one to the other,
tests/test_world_changes_gpu.py the library to BrickModel.  Both sides of a cell are classified by world_ref.writes, the
archive's own rule.  World cells are (x, y, z); brick = cell >> 3; a brick's cell word is cx | cy << 3 | cz << 6; a word is
track | label << 16 | occ << 24."""
import collections
import itertools

import numpy as np

from semantic_dsp_map_amd.binding import (ALL_CHANGE_CLASSES, ALL_LABELS, WORLD_CHANGE_APPEARED, WORLD_CHANGE_NONE, WORLD_CHANGE_REGION,
                                          WORLD_CHANGE_RELABELLED, WORLD_CHANGE_RESULT, WORLD_CHANGE_UNLISTED, WORLD_CHANGE_VANISHED,
                                          WORLD_CHANGES_BY_LABEL, WORLD_CHANGES_COUNTERS, WORLD_CHANGES_FACE_CONNECTED, WORLD_CHANGES_INFO,
                                          WORLD_CHANGES_OBSERVED_ONLY, WORLD_CHANGES_OLDER, WORLD_CHANGES_STATIC_ONLY)
from tests import world_ref as wr

B_MIN, B_MAX = -32768, 32767
UNKNOWN = wr.UNKNOWN
AROUND = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
U, F, O = 0, 1, 2


def flags_of(face_connected=False, by_label=False, static_only=False, observed_only=False, max_last_stamp=None):
    return ((WORLD_CHANGES_FACE_CONNECTED if face_connected else 0) | (WORLD_CHANGES_BY_LABEL if by_label else 0) |
            (WORLD_CHANGES_STATIC_ONLY if static_only else 0) | (WORLD_CHANGES_OBSERVED_ONLY if observed_only else 0) |
            (WORLD_CHANGES_OLDER if max_last_stamp is not None else 0))


def in_range(b):
    return all(B_MIN <= int(v) <= B_MAX for v in b)


def side_class(words, max_movable, static_only, observed_only):
    """U, F or O per word: a word is known iff it would write under the archive's rule with the layer's flags"""
    w = np.asarray(words, np.uint32)
    known = wr.writes(w, max_movable, (wr.STATIC_ONLY if static_only else 0) | (wr.OBSERVED_ONLY if observed_only else 0))
    return np.where(known, np.where(wr.occ_of(w) >= 1, O, F), U)


def classify(now, before, max_movable, static_only, observed_only):
    """-> (class per cell: 0 or the three change classes, the eight counters of the class table as a dict of masks)"""
    now, before = np.asarray(now, np.uint32), np.asarray(before, np.uint32)
    sn, sb = side_class(now, max_movable, static_only, observed_only), side_class(before, max_movable, static_only, observed_only)
    ln, lb = (now >> 16) & 0xFF, (before >> 16) & 0xFF
    cls = np.zeros(now.shape, np.int64)
    cls[(sn == O) & (sb == F)] = WORLD_CHANGE_APPEARED
    cls[(sn == F) & (sb == O)] = WORLD_CHANGE_VANISHED
    cls[(sn == O) & (sb == O) & (ln != lb)] = WORLD_CHANGE_RELABELLED
    masks = dict(n_appeared=cls == WORLD_CHANGE_APPEARED, n_vanished=cls == WORLD_CHANGE_VANISHED, n_relabelled=cls == WORLD_CHANGE_RELABELLED,
                 n_same_occupied=(sn == O) & (sb == O) & (ln == lb), n_same_free=(sn == F) & (sb == F), n_new_occupied=(sn == O) & (sb == U),
                 n_new_free=(sn == F) & (sb == U), n_remembered=(sn == U) & (sb != U), n_known_now=sn != U, n_known_before=sb != U)
    return cls, masks


def listed_of(cls, now, before, labels, classes):
    """which changed cells are listed: the class's bit, and one of the occupied sides' labels admitted"""
    admit = np.zeros(256, bool)
    admit[[int(l) for l in labels]] = True
    wanted = np.zeros(4, bool)
    wanted[[int(c) for c in classes]] = True
    a_now, a_before = admit[(np.asarray(now, np.uint32) >> 16) & 0xFF], admit[(np.asarray(before, np.uint32) >> 16) & 0xFF]
    return (cls != 0) & wanted[cls] & (((cls != WORLD_CHANGE_VANISHED) & a_now) | ((cls != WORLD_CHANGE_APPEARED) & a_before))


def pair_of(now, before, cls):
    """label_now << 8 | label_before << 16, a side that is not occupied reading 0"""
    now, before, cls = np.asarray(now, np.int64), np.asarray(before, np.int64), np.asarray(cls, np.int64)
    ln = np.where(cls != WORLD_CHANGE_VANISHED, (now >> 16) & 0xFF, 0)
    lb = np.where(cls != WORLD_CHANGE_APPEARED, (before >> 16) & 0xFF, 0)
    return (ln << 8) | (lb << 16)


def archive_of(hdr, cells, max_last_stamp):
    """brick (bx, by, bz) -> its 512 words, of the bricks the build may compare"""
    out = {}
    for j in range(len(hdr)):
        b = (int(hdr["bx"][j]), int(hdr["by"][j]), int(hdr["bz"][j]))
        if max_last_stamp is not None and int(hdr["last_stamp"][j]) > int(max_last_stamp):
            continue
        out[b] = np.asarray(cells[j], np.uint32).reshape(512)
    return out


def bits_of(word):
    out = []
    while word:
        low = word & -word
        out.append(low.bit_length() - 1)
        word ^= low
    return out


def word_of(mask64):
    """bool [64] -> a Python int, bit cx + 8 cy"""
    return int((np.asarray(mask64, bool).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(dtype=np.uint64))


class _Common:
    """from the cell list with its words and classes and a component label per cell (the index of the component's first
    cell): the region index per cell, the table, the per-label counters and the info record"""

    def _finish(self, coords, cells, now, before, cls, label, counters, n_candidates, voxel_size, min_cells, flags, frame_stamp, stamp):
        n = len(cells)
        self.coords = np.asarray(coords, np.int64).reshape(-1, 3)
        self.cells = np.asarray(cells, np.int64).reshape(-1, 3).astype(np.int32)
        self.now, self.before = np.asarray(now, np.uint32).reshape(-1), np.asarray(before, np.uint32).reshape(-1)
        self.cls = np.asarray(cls, np.uint8).reshape(-1)
        label = np.asarray(label, np.int64).reshape(-1)
        assert n == 0 or ((label <= np.arange(n)).all() and (label[label] == label).all())
        roots = np.flatnonzero(label == np.arange(n)) if n else np.zeros(0, np.int64)
        size = np.bincount(label, minlength=n)[roots] if n else np.zeros(0, np.int64)
        listed = roots[size >= max(int(min_cells), 1)]
        place = np.full(n + 1, WORLD_CHANGE_UNLISTED, np.int64)
        place[listed] = np.arange(len(listed))
        self.region = place[label].astype(np.uint32) if n else np.zeros(0, np.uint32)
        pair = pair_of(self.now, self.before, self.cls)
        size32 = np.float32(voxel_size)
        t = np.zeros(len(listed), WORLD_CHANGE_REGION)
        wide = self.cells.astype(np.int64)
        for k, r in enumerate(listed.tolist()):
            rows = np.flatnonzero(label == r)
            mine = wide[rows]
            lo, hi, total = mine.min(axis=0), mine.max(axis=0), mine.sum(axis=0)
            t[k]["first_index"], t[k]["n_cells"], t[k]["cls"] = r, len(mine), self.cls[r]
            t[k]["label_now"], t[k]["label_before"] = (int(pair[r]) >> 8) & 0xFF, (int(pair[r]) >> 16) & 0xFF
            t[k]["mixed"] = int((pair[rows] != pair[r]).any())
            t[k]["first_cell"], t[k]["cell_min"], t[k]["cell_max"], t[k]["cell_sum"] = wide[r], lo, hi, total
            t[k]["box_min"] = lo.astype(np.float32) * size32
            t[k]["box_max"] = (hi + 1).astype(np.float32) * size32
            t[k]["centroid"] = ((total.astype(np.float64) / np.float64(len(mine)) + np.float64(0.5)) * np.float64(size32)).astype(np.float32)
        self.table = t
        lab_now, lab_before = ((self.now >> 16) & 0xFF).astype(np.int64), ((self.before >> 16) & 0xFF).astype(np.int64)
        self.appeared = np.bincount(lab_now[self.cls == WORLD_CHANGE_APPEARED], minlength=256).astype(np.uint64)
        self.vanished = np.bincount(lab_before[self.cls == WORLD_CHANGE_VANISHED], minlength=256).astype(np.uint64)
        self.relabelled = np.bincount(lab_now[self.cls == WORLD_CHANGE_RELABELLED], minlength=256).astype(np.uint64)
        self.info = np.zeros(1, WORLD_CHANGES_INFO)[0]
        for name in WORLD_CHANGES_COUNTERS:
            self.info[name] = counters[name]
        self.info["n_candidates"], self.info["n_bricks"], self.info["n_cells"] = n_candidates, len(self.coords), n
        self.info["n_regions"], self.info["n_regions_total"], self.info["flags"], self.info["min_cells"] = len(listed), len(roots), flags, min_cells
        self.info["frame_stamp"], self.info["stamp"] = frame_stamp, stamp
        self._index = None

    def query(self, cells=None, xyz=None, voxel_size=None):
        """WORLD_CHANGE_RESULT per world cell, or per point (float32 [n, 3]; the archive's rule: floorf(p * recip))"""
        if self._index is None:
            self._index = {tuple(c): i for i, c in enumerate(self.cells.tolist())}
        if cells is not None:
            g = np.asarray(cells, np.int64).reshape(-1, 3)
            ok = np.array([in_range((int(c[0]) >> 3, int(c[1]) >> 3, int(c[2]) >> 3)) for c in g], bool).reshape(-1)
        else:
            p = np.asarray(xyz, np.float32).reshape(-1, 3)
            recip = np.float32(1.0) / np.float32(voxel_size)
            with np.errstate(all="ignore"):
                v = np.floor(p * recip)
                ok = ((v >= -262144.0) & (v < 262144.0)).all(axis=1)
            g = np.where(ok[:, None], np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)
        out = np.zeros(len(g), WORLD_CHANGE_RESULT)
        out["cell"] = g
        out["region"], out["index"], out["cls"] = WORLD_CHANGE_NONE, WORLD_CHANGE_NONE, WORLD_CHANGE_NONE
        for i, c in enumerate(g.tolist()):
            at = self._index.get(tuple(c)) if ok[i] else None
            if at is not None:
                out[i]["index"], out[i]["region"], out[i]["cls"] = at, self.region[at], self.cls[at]
        return out


def _keys(now, before, cls, by_label):
    cls = np.asarray(cls, np.int64)
    return (cls | pair_of(now, before, cls)) if by_label else cls


class BrickModel(_Common):
    def __init__(self, snap, moved_steps, frame_stamp, hdr, cells, stamp, voxel_size, max_movable, face_connected=False, by_label=False,
                 static_only=False, observed_only=False, max_last_stamp=None, labels=ALL_LABELS, classes=ALL_CHANGE_CLASSES, min_cells=1):
        snap = np.asarray(snap, np.uint32)
        b0, nb, block = wr.brick_view(snap, moved_steps)
        arch = archive_of(hdr, cells, max_last_stamp)
        nc = len(block)
        counters = dict.fromkeys(WORLD_CHANGES_COUNTERS, 0)
        counters["n_outside"] = nc * 512 - snap.size
        coords, cw, pre, out_cells, out_now, out_before, out_cls = [], [], [0], [], [], [], []
        for c in range(nc):                                      # ascending candidate index = brick order
            t, kx = divmod(c, int(nb[0]))
            kz, ky = divmod(t, int(nb[1]))
            b = (int(b0[0]) + kx, int(b0[1]) + ky, int(b0[2]) + kz)
            before = arch.get(b) if in_range(b) else None
            if before is None:
                before = np.full(512, UNKNOWN, np.uint32)
            cls, masks = classify(block[c], before, max_movable, static_only, observed_only)
            for name, m in masks.items():
                counters[name] += int(m.sum())
            listed = listed_of(cls, block[c], before, labels, classes)
            if not listed.any():
                continue
            coords.append(b)
            words = [word_of(listed[z * 64:z * 64 + 64]) for z in range(8)]
            cw.append(words)
            for z in range(8):
                pre.append(pre[-1] + bin(words[z]).count("1"))
                for bit in bits_of(words[z]):
                    w = z * 64 + bit
                    out_cells.append((b[0] * 8 + (bit & 7), b[1] * 8 + (bit >> 3), b[2] * 8 + z))
                    out_now.append(int(block[c][w])), out_before.append(int(before[w])), out_cls.append(int(cls[w]))
        total = pre[-1]
        rank_of = {b: r for r, b in enumerate(coords)}
        key_at = _keys(np.array(out_now, np.uint32), np.array(out_before, np.uint32), np.array(out_cls, np.int64), by_label).tolist() if total else []
        parent = list(range(total))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        def index_of(r, x, y, z):
            """the list index of cell (x, y, z) of field brick r, None if it is no listed cell"""
            bit = x + 8 * y
            w = cw[r][z]
            return pre[r * 8 + z] + bin(w & ((1 << bit) - 1)).count("1") if (w >> bit) & 1 else None

        moves = [d for d in AROUND if not face_connected or sum(v != 0 for v in d) == 1]
        for r, b in enumerate(coords):
            for z in range(8):
                for bit in bits_of(cw[r][z]):
                    lx, ly = bit & 7, bit >> 3
                    a = index_of(r, lx, ly, z)
                    for d in moves:
                        x, y, zz = lx + d[0], ly + d[1], z + d[2]
                        nr = rank_of.get((b[0] + (x >> 3), b[1] + (y >> 3), b[2] + (zz >> 3)))
                        if nr is None:
                            continue
                        o = index_of(nr, x & 7, y & 7, zz & 7)
                        if o is not None and o < a and key_at[o] == key_at[a]:
                            ra, ro = find(a), find(o)
                            if ra != ro:
                                parent[max(ra, ro)] = min(ra, ro)   # the root of a component is its smallest index
        label = [find(a) for a in range(total)]
        flags = flags_of(face_connected, by_label, static_only, observed_only, max_last_stamp)
        self._finish(coords, out_cells, out_now, out_before, out_cls, label, counters, nc, voxel_size, min_cells, flags, frame_stamp, stamp)


class CellModel(_Common):
    def __init__(self, snap, moved_steps, frame_stamp, hdr, cells, stamp, voxel_size, max_movable, face_connected=False, by_label=False,
                 static_only=False, observed_only=False, max_last_stamp=None, labels=ALL_LABELS, classes=ALL_CHANGE_CLASSES, min_cells=1):
        snap = np.asarray(snap, np.uint32)
        N = np.array(snap.shape[::-1], np.int64)
        g0 = wr.block_origin(snap, moved_steps)
        lo, hi = (g0 >> 3) * 8, ((g0 + N - 1) >> 3) * 8 + 8           # the candidates' box in world cells, hi exclusive
        ext = (hi - lo).astype(np.int64)
        now = np.full((ext[2], ext[1], ext[0]), UNKNOWN, np.uint32)
        inside = np.zeros(now.shape, bool)
        o = g0 - lo
        now[o[2]:o[2] + N[2], o[1]:o[1] + N[1], o[0]:o[0] + N[0]] = snap
        inside[o[2]:o[2] + N[2], o[1]:o[1] + N[1], o[0]:o[0] + N[0]] = True
        before = np.full(now.shape, UNKNOWN, np.uint32)
        for b, words in archive_of(hdr, cells, max_last_stamp).items():
            at = np.array(b, np.int64) * 8 - lo
            if in_range(b) and (at >= 0).all() and (at < ext).all():
                before[at[2]:at[2] + 8, at[1]:at[1] + 8, at[0]:at[0] + 8] = words.reshape(8, 8, 8)
        cls, masks = classify(now, before, max_movable, static_only, observed_only)
        counters = {name: int(m.sum()) for name, m in masks.items()}
        counters["n_outside"] = int((~inside).sum())
        listed = listed_of(cls, now, before, labels, classes)
        z, y, x = np.nonzero(listed)
        g = np.stack([x + lo[0], y + lo[1], z + lo[2]], 1)
        order = sorted(range(len(g)), key=lambda i: (g[i][2] >> 3, g[i][1] >> 3, g[i][0] >> 3, (g[i][0] & 7) | (g[i][1] & 7) << 3 | (g[i][2] & 7) << 6))
        out_cells = [tuple(int(v) for v in g[i]) for i in order]
        out_now, out_before, out_cls = now[z, y, x][order], before[z, y, x][order], cls[z, y, x][order]
        coords = sorted({(c[0] >> 3, c[1] >> 3, c[2] >> 3) for c in out_cells}, key=lambda b: (b[2], b[1], b[0]))
        index = {c: i for i, c in enumerate(out_cells)}
        key_at = _keys(out_now, out_before, out_cls, by_label).tolist() if out_cells else []
        moves = [d for d in AROUND if not face_connected or sum(v != 0 for v in d) == 1]
        label = [-1] * len(out_cells)
        for i, c in enumerate(out_cells):                    # in list order: a component is found from its first cell
            if label[i] >= 0:
                continue
            label[i] = i
            todo = collections.deque([c])
            while todo:
                p = todo.popleft()
                for d in moves:
                    q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                    k = index.get(q)
                    if k is not None and label[k] < 0 and key_at[k] == key_at[i]:
                        label[k] = i
                        todo.append(q)
        nc = int(np.prod(ext // 8))
        flags = flags_of(face_connected, by_label, static_only, observed_only, max_last_stamp)
        self._finish(coords, out_cells, out_now, out_before, out_cls, label, counters, nc, voxel_size, min_cells, flags, frame_stamp, stamp)


NAMES = ("cells", "now", "before", "cls", "region", "table", "appeared", "vanished", "relabelled", "info")


def answer(model):
    return (model.cells, model.now, model.before, model.cls, model.region, model.table, model.appeared, model.vanished, model.relabelled,
            model.info)


def difference(got, want):
    """None, or what differs between two answers - models or the library's getters"""
    for name, a, b in zip(NAMES, got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            return "%s: shape / dtype %s %s against %s %s" % (name, a.shape, a.dtype, b.shape, b.dtype)
        if a.tobytes() != b.tobytes():
            if a.dtype.names:
                bad = [f for f in a.dtype.names if a[f].tobytes() != b[f].tobytes()]
                return "%s: fields %s differ: %s against %s" % (name, bad, a[bad[0]].reshape(-1)[:6], b[bad[0]].reshape(-1)[:6])
            at = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
            return "%s: %d rows differ, first %d: %s against %s" % (name, len(at), at[0], a[at[0]], b[at[0]])
    return None
