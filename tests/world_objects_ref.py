"""NumPy / Python restatement of the world objects (include/sdm.h: sdm_world_objects_update / sdm_get_world_objects /
sdm_get_world_object_cells / sdm_get_world_object_labels / sdm_query_world_objects), for the tests.  No SciPy.  Written twice:

  * BrickModel: per brick and key eight 64-bit layer words (bit cx + 8 cy) of the counted cells; a brick's components are
    found by growing a seed with shifts inside the words - x by one bit with the wrapping column masked, y by eight bits,
    z the word above or below - and masking with the key's words; the cell list is the counted words' bits in order; the
    objects are a union-find over the cells' ranks in two passes - inside each brick, then across the seams from the cells
    on a brick's shell, where the keys are compared.  `separable=True` masks after every 1-D stage of the 3 x 3 x 3 growth,
    `wrap_mask=False` leaves out the column masks of the x shifts and `seams=False` the second pass: what the tests show
    such a model to get wrong.
  * CellModel: a dict from world cell to word over the field, a breadth-first search over the counted cells in list order
    that steps only to counted cells of an equal key.

Both take what a caller can read back - world_bricks() - and give the cell list with the words, the object index per cell,
the table, the per-label counters and the info block; tests/test_world_objects_ref.py holds one to the other,
tests/test_world_objects_gpu.py the library to BrickModel.  World cells are (x, y, z); brick = cell >> 3; a brick's cell
word is cx | cy << 3 | cz << 6; an archived word is track | label << 16 | occ << 24."""
import collections
import itertools

import numpy as np

from semantic_dsp_map_amd.binding import (ALL_LABELS, WORLD_OBJECT, WORLD_OBJECT_NONE, WORLD_OBJECT_RESULT, WORLD_OBJECT_UNLISTED, WORLD_OBJECTS_BOX,
                                          WORLD_OBJECTS_BY_TRACK, WORLD_OBJECTS_FACE_CONNECTED, WORLD_OBJECTS_INFO, WORLD_OBJECTS_MOVABLE_ONLY,
                                          WORLD_OBJECTS_OBSERVED_ONLY, WORLD_OBJECTS_STATIC_ONLY)

B_MIN, B_MAX = -32768, 32767
ALL = (1 << 64) - 1
COL0, COL7 = 0x0101010101010101, 0x8080808080808080
AROUND = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
LOCAL = [(w & 7, (w >> 3) & 7, w >> 6) for w in range(512)]


def flags_of(face_connected=False, by_track=False, static_only=False, movable_only=False, observed_only=False, box=None):
    return ((WORLD_OBJECTS_FACE_CONNECTED if face_connected else 0) | (WORLD_OBJECTS_BOX if box is not None else 0) |
            (WORLD_OBJECTS_BY_TRACK if by_track else 0) | (WORLD_OBJECTS_STATIC_ONLY if static_only else 0) |
            (WORLD_OBJECTS_MOVABLE_ONLY if movable_only else 0) | (WORLD_OBJECTS_OBSERVED_ONLY if observed_only else 0))


def brick_coords(hdr):
    coord = np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int64).reshape(-1, 3)
    order = np.lexsort((coord[:, 0], coord[:, 1], coord[:, 2]))
    assert np.array_equal(order, np.arange(len(coord))), "world_bricks() is in brick order"
    return coord


def in_box(coord, box):
    if box is None:
        return np.ones(len(coord), bool)
    return ((coord >= np.asarray(box[0], np.int64)) & (coord <= np.asarray(box[1], np.int64))).all(axis=1).reshape(-1)


def in_range(b):
    return all(B_MIN <= v <= B_MAX for v in b)


def counted(words, max_movable, static_only=False, movable_only=False, observed_only=False, labels=ALL_LABELS):
    """bool, like words: which archived words are counted cells"""
    w = np.asarray(words, np.uint32)
    occ = ((w >> 24) & 0xFF).astype(np.uint8).view(np.int8)
    track, label = w & 0xFFFF, (w >> 16) & 0xFF
    movable = (track >= 1) & (track <= max_movable)
    admit = np.zeros(256, bool)
    admit[[int(l) for l in labels]] = True
    ok = (occ >= 1) & admit[label]
    if static_only:
        ok &= ~movable
    if movable_only:
        ok &= movable
    if observed_only:
        ok &= occ != 2
    return ok


def keys_of(words, by_track):
    w = np.asarray(words, np.uint32)
    return (w & 0xFFFFFF) if by_track else ((w >> 16) & 0xFF)


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
    """from the cell list, the words and a component label per cell (the index of the component's first cell): the object
    index per cell, the table, the per-label counters and the info block"""

    def _finish(self, coords, cells, words, label, voxel_size, min_cells, flags, stamp):
        n = len(cells)
        self.coords = coords
        self.cells = np.asarray(cells, np.int64).reshape(-1, 3).astype(np.int32)
        self.words = np.asarray(words, np.uint32).reshape(-1)
        label = np.asarray(label, np.int64).reshape(-1)
        assert n == 0 or ((label <= np.arange(n)).all() and (label[label] == label).all())
        roots = np.flatnonzero(label == np.arange(n)) if n else np.zeros(0, np.int64)
        size = np.bincount(label, minlength=n)[roots] if n else np.zeros(0, np.int64)
        listed = roots[size >= max(int(min_cells), 1)]
        place = np.full(n + 1, WORLD_OBJECT_UNLISTED, np.int64)
        place[listed] = np.arange(len(listed))
        self.object = place[label].astype(np.uint32) if n else np.zeros(0, np.uint32)
        size32 = np.float32(voxel_size)
        t = np.zeros(len(listed), WORLD_OBJECT)
        wide = self.cells.astype(np.int64)
        occ = (self.words >> 24) & 0xFF
        order = np.argsort(label, kind="stable") if n else np.zeros(0, np.int64)
        starts = np.searchsorted(label[order], listed) if n else np.zeros(0, np.int64)
        sizes = dict(zip(roots.tolist(), size.tolist()))
        for k, r in enumerate(listed.tolist()):
            rows = order[starts[k]:starts[k] + sizes[r]]
            mine = wide[rows]
            lo, hi, total = mine.min(axis=0), mine.max(axis=0), mine.sum(axis=0)
            t[k]["first_index"], t[k]["n_cells"], t[k]["n_guessed"] = r, len(mine), int((occ[rows] == 2).sum())
            t[k]["track"], t[k]["label"] = int(self.words[r]) & 0xFFFF, (int(self.words[r]) >> 16) & 0xFF
            t[k]["mixed_tracks"] = int(((self.words[rows] & 0xFFFF) != (self.words[r] & 0xFFFF)).any())
            t[k]["first_cell"], t[k]["cell_min"], t[k]["cell_max"], t[k]["cell_sum"] = wide[r], lo, hi, total
            d = [[int(v) for v in row] for row in (mine - wide[r]).tolist()]       # Python ints: no silent wrap
            sq = [sum(p[a] * p[b] for p in d) & ALL for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
            t[k]["cell_sq"] = np.array(sq, np.uint64).view(np.int64)
            t[k]["box_min"] = lo.astype(np.float32) * size32
            t[k]["box_max"] = (hi + 1).astype(np.float32) * size32
            t[k]["centroid"] = ((total.astype(np.float64) / np.float64(len(mine)) + np.float64(0.5)) * np.float64(size32)).astype(np.float32)
        self.table = t
        lab = ((self.words >> 16) & 0xFF).astype(np.int64)
        self.label_cells = np.bincount(lab, minlength=256).astype(np.uint64)
        self.label_objects = np.bincount(lab[roots], minlength=256).astype(np.uint32)
        self.info = np.zeros(1, WORLD_OBJECTS_INFO)[0]
        self.info["n_bricks"], self.info["n_objects"], self.info["n_objects_total"], self.info["flags"] = len(coords), len(listed), len(roots), flags
        self.info["n_cells"], self.info["n_guessed"], self.info["min_cells"], self.info["stamp"] = n, int((occ == 2).sum()), min_cells, stamp
        self._index = None

    def query(self, cells=None, xyz=None, voxel_size=None):
        """WORLD_OBJECT_RESULT per world cell, or per point (float32 [n, 3]; the archive's rule: floorf(p * recip))"""
        if self._index is None:
            self._index = {tuple(c): i for i, c in enumerate(self.cells.tolist())}
        if cells is not None:
            g = np.asarray(cells, np.int64).reshape(-1, 3)
            ok = np.array([in_range((int(c[0]) >> 3, int(c[1]) >> 3, int(c[2]) >> 3)) for c in g], bool).reshape(-1)
            echo = g
        else:
            p = np.asarray(xyz, np.float32).reshape(-1, 3)
            recip = np.float32(1.0) / np.float32(voxel_size)
            with np.errstate(all="ignore"):
                v = np.floor(p * recip)
                ok = ((v >= -262144.0) & (v < 262144.0)).all(axis=1)
            g = np.where(ok[:, None], np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)
            echo = g
        out = np.zeros(len(g), WORLD_OBJECT_RESULT)
        out["cell"] = echo
        out["object"], out["index"] = WORLD_OBJECT_NONE, WORLD_OBJECT_NONE
        for i, c in enumerate(g.tolist()):
            at = self._index.get(tuple(c)) if ok[i] else None
            if at is not None:
                out[i]["index"], out[i]["object"] = at, self.object[at]
        return out


class BrickModel(_Common):
    def __init__(self, hdr, cells, voxel_size, max_movable, face_connected=False, by_track=False, static_only=False, movable_only=False,
                 observed_only=False, labels=ALL_LABELS, box=None, min_cells=1, stamp=0, separable=False, wrap_mask=True, seams=True):
        coord = brick_coords(hdr)
        words = np.asarray(cells, np.uint32).reshape(-1, 512)
        field = np.flatnonzero(in_box(coord, box))
        rank_of = {tuple(coord[j].tolist()): r for r, j in enumerate(field.tolist())}     # the field only: nothing else joins
        n = len(field)
        not0, not7 = (ALL & ~COL0, ALL & ~COL7) if wrap_mask else (ALL, ALL)

        def x_grow(w):
            return w | ((w << 1) & not0 & ALL) | ((w >> 1) & not7)

        def y_grow(w):
            return w | ((w << 8) & ALL) | (w >> 8)

        def grow(s, key_words):
            """the cells of the key next to the set s (eight words), s included"""
            if face_connected:
                g = [x_grow(s[z]) | y_grow(s[z]) | (s[z - 1] if z > 0 else 0) | (s[z + 1] if z < 7 else 0) for z in range(8)]
                return [g[z] & key_words[z] for z in range(8)]
            g = [x_grow(s[z]) for z in range(8)]
            if separable:
                g = [g[z] & key_words[z] for z in range(8)]
            g = [y_grow(g[z]) for z in range(8)]
            if separable:
                g = [g[z] & key_words[z] for z in range(8)]
            g = [g[z] | (g[z - 1] if z > 0 else 0) | (g[z + 1] if z < 7 else 0) for z in range(8)]
            return [g[z] & key_words[z] for z in range(8)]

        cw = [[0] * 8 for _ in range(n)]
        pre = np.zeros(n * 8 + 1, np.int64)
        out_cells, out_words, local = [], [], []     # local: per brick its components, eight words each
        for r in range(n):
            j = int(field[r])
            ok = counted(words[j], max_movable, static_only, movable_only, observed_only, labels)
            keys = keys_of(words[j], by_track)
            comps = []
            for key in np.unique(keys[ok]).tolist():
                kw = [word_of((ok & (keys == key))[z * 64:z * 64 + 64]) for z in range(8)]
                for z in range(8):
                    cw[r][z] |= kw[z]
                left = list(kw)
                while any(left):
                    z0 = next(z for z in range(8) if left[z])
                    s = [0] * 8
                    s[z0] = left[z0] & -left[z0]
                    while True:
                        g = grow(s, kw)
                        if g == s:
                            break
                        s = g
                    comps.append(s)
                    left = [left[z] & ~s[z] for z in range(8)]
            local.append(comps)
            for z in range(8):
                pre[r * 8 + z + 1] = pre[r * 8 + z] + bin(cw[r][z]).count("1")
                for bit in bits_of(cw[r][z]):
                    out_cells.append((coord[j][0] * 8 + (bit & 7), coord[j][1] * 8 + (bit >> 3), coord[j][2] * 8 + z))
                    out_words.append(int(words[j][z * 64 + bit]))
        total = int(pre[-1])
        parent = list(range(total))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        def unite(a, b):
            a, b = find(a), find(b)
            if a != b:
                parent[max(a, b)] = min(a, b)   # the root of a component is its smallest rank

        def index_of(r, x, y, z):
            """the rank of cell (x, y, z) of field brick r, None if it is no counted cell"""
            bit = x + 8 * y
            w = cw[r][z]
            return int(pre[r * 8 + z]) + bin(w & ((1 << bit) - 1)).count("1") if (w >> bit) & 1 else None

        for r in range(n):                                   # inside a brick: every cell of a component to its first
            for s in local[r]:
                ranks = [index_of(r, bit & 7, bit >> 3, z) for z in range(8) for bit in bits_of(s[z])]
                for a in ranks[1:]:
                    unite(ranks[0], a)
        key_at = keys_of(np.array(out_words, np.uint32), by_track).tolist() if total else []
        moves = [d for d in AROUND if not face_connected or sum(v != 0 for v in d) == 1]
        if seams:                                            # across the seams, from the shell
            for r in range(n):
                b = coord[int(field[r])].tolist()
                for z in range(8):
                    for bit in bits_of(cw[r][z]):
                        lx, ly = bit & 7, bit >> 3
                        if not (lx in (0, 7) or ly in (0, 7) or z in (0, 7)):
                            continue
                        a = index_of(r, lx, ly, z)
                        for d in moves:
                            x, y, zz = lx + d[0], ly + d[1], z + d[2]
                            q = (b[0] + (x >> 3), b[1] + (y >> 3), b[2] + (zz >> 3))
                            if q == tuple(b) or not in_range(q):
                                continue
                            nr = rank_of.get(q)
                            if nr is None or nr > r:
                                continue
                            o = index_of(nr, x & 7, y & 7, zz & 7)
                            if o is not None and key_at[o] == key_at[a]:
                                unite(a, o)
        label = [find(a) for a in range(total)]
        flags = flags_of(face_connected, by_track, static_only, movable_only, observed_only, box)
        self._finish(coord[field], out_cells, out_words, label, voxel_size, min_cells, flags, stamp)


class CellModel(_Common):
    def __init__(self, hdr, cells, voxel_size, max_movable, face_connected=False, by_track=False, static_only=False, movable_only=False,
                 observed_only=False, labels=ALL_LABELS, box=None, min_cells=1, stamp=0):
        coord = brick_coords(hdr)
        words = np.asarray(cells, np.uint32).reshape(-1, 512)
        field = np.flatnonzero(in_box(coord, box))
        out_cells, out_words = [], []
        for j in field.tolist():
            b = coord[j].tolist()
            if not in_range(b):
                continue
            ok = counted(words[j], max_movable, static_only, movable_only, observed_only, labels)
            for w in np.flatnonzero(ok).tolist():
                out_cells.append((b[0] * 8 + LOCAL[w][0], b[1] * 8 + LOCAL[w][1], b[2] * 8 + LOCAL[w][2]))
                out_words.append(int(words[j][w]))
        index = {c: i for i, c in enumerate(out_cells)}
        key_at = keys_of(np.array(out_words, np.uint32), by_track).tolist() if out_cells else []
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
        flags = flags_of(face_connected, by_track, static_only, movable_only, observed_only, box)
        self._finish(coord[field], out_cells, out_words, label, voxel_size, min_cells, flags, stamp)


def difference(got, want):
    """None, or what differs between two (cells, object, words, table, label_cells, label_objects, info) answers - models or
    the library's getters"""
    names = ("cells", "object", "words", "table", "label_cells", "label_objects", "info")
    for name, a, b in zip(names, got, want):
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


def answer(model):
    return model.cells, model.object, model.words, model.table, model.label_cells, model.label_objects, model.info
