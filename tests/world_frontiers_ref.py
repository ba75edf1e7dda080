"""NumPy restatement of the world frontiers (include/sdm.h: sdm_world_frontiers_update / sdm_get_world_frontier_clusters /
sdm_get_world_frontier_cells), for the tests.  No SciPy.  Written twice:

  * BrickModel: per brick eight 64-bit layer words (bit cx + 8 cy) of `free` and `unknown`; the frontier word of a layer
    is free & (unknown at x-1 | x+1 | y-1 | y+1 | z-1 | z+1) by shifts inside the word, the wrapping column masked and
    the neighbour brick's column, row or word brought in; the cell list is the words' bits in order; the clusters are a
    union-find over the cells' ranks in two passes - inside each brick, then across the seams from the cells on a brick's
    shell.  `seams=False` leaves the second pass out and `wrap_mask=False` the column masks of the x shifts: what the
    tests show such a model to get wrong.
  * CellModel: a dict from world cell to word over the whole archive, a plain test of the six neighbours cell by cell, a
    breadth-first search over the frontier cells in list order.

Both take what a caller can read back - world_bricks() - and give the cell list, unknown_faces, the cluster index per
cell, the cluster table and the info block; tests/test_world_frontiers_ref.py holds one to the other,
tests/test_world_frontiers_gpu.py the library to BrickModel.  World cells are (x, y, z); brick = cell >> 3; a brick's
cell word is cx | cy << 3 | cz << 6."""
import collections
import itertools

import numpy as np

from semantic_dsp_map_amd.binding import (WORLD_FRONTIER_CLUSTER, WORLD_FRONTIER_NO_CLUSTER, WORLD_FRONTIERS_BOX, WORLD_FRONTIERS_FACE_CONNECTED,
                                          WORLD_FRONTIERS_INFO, WORLD_FRONTIERS_INSIDE_BRICKS)

B_MIN, B_MAX = -32768, 32767
ALL = (1 << 64) - 1
COL0, COL7 = 0x0101010101010101, 0x8080808080808080
ROW0, ROW7 = 0xFF, 0xFF << 56
FACES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
AROUND = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]


def occ_of(words):
    return ((np.asarray(words, np.uint32) >> 24) & 0xFF).astype(np.uint8).view(np.int8)


def flags_of(face_connected=False, box=None, inside_bricks=False):
    return ((WORLD_FRONTIERS_FACE_CONNECTED if face_connected else 0) | (WORLD_FRONTIERS_BOX if box is not None else 0) |
            (WORLD_FRONTIERS_INSIDE_BRICKS if inside_bricks else 0))


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


class _Common:
    """from the cell list, unknown_faces and a component label per cell (the index of the component's first cell): the
    cluster index per cell, the table and the info block"""

    def _finish(self, n_bricks, cells, faces, label, n_absent, voxel_size, min_cells, flags, stamp):
        n = len(cells)
        self.cells = np.asarray(cells, np.int64).reshape(-1, 3).astype(np.int32)
        self.faces = np.asarray(faces, np.int64).astype(np.uint8)
        label = np.asarray(label, np.int64)
        assert n == 0 or ((label <= np.arange(n)).all() and (label[label] == label).all())
        roots = np.flatnonzero(label == np.arange(n)) if n else np.zeros(0, np.int64)
        size = np.bincount(label, minlength=n)[roots] if n else np.zeros(0, np.int64)
        listed = roots[size >= max(int(min_cells), 1)]
        place = np.full(n + 1, WORLD_FRONTIER_NO_CLUSTER, np.int64)
        place[listed] = np.arange(len(listed))
        self.cluster = place[label].astype(np.uint32) if n else np.zeros(0, np.uint32)
        size32 = np.float32(voxel_size)
        t = np.zeros(len(listed), WORLD_FRONTIER_CLUSTER)
        wide = self.cells.astype(np.int64)
        for k, r in enumerate(listed.tolist()):
            mine = wide[label == r]
            lo, hi, total = mine.min(axis=0), mine.max(axis=0), mine.sum(axis=0)
            t[k]["first_index"], t[k]["n_cells"], t[k]["n_unknown_faces"] = r, len(mine), int(self.faces[label == r].astype(np.int64).sum())
            t[k]["first_cell"], t[k]["cell_min"], t[k]["cell_max"], t[k]["cell_sum"] = wide[r], lo, hi, total
            t[k]["box_min"] = lo.astype(np.float32) * size32
            t[k]["box_max"] = (hi + 1).astype(np.float32) * size32
            t[k]["centroid"] = ((total.astype(np.float64) / np.float64(len(mine)) + np.float64(0.5)) * np.float64(size32)).astype(np.float32)
        self.table = t
        self.info = np.zeros(1, WORLD_FRONTIERS_INFO)[0]
        self.info["n_bricks"], self.info["n_clusters"], self.info["n_clusters_total"], self.info["flags"] = n_bricks, len(listed), len(roots), flags
        self.info["n_cells"], self.info["n_unknown_faces"], self.info["n_absent_faces"] = n, int(self.faces.astype(np.int64).sum()), n_absent
        self.info["min_cells"], self.info["stamp"] = min_cells, stamp


def layer_words(mask):
    """bool [n, 512] -> Python ints [n][8]: bit cx + 8 cy of layer cz"""
    m = np.asarray(mask, bool).reshape(-1, 8, 64)
    w = (m.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    return [[int(v) for v in row] for row in w]


def bits_of(word):
    out = []
    while word:
        low = word & -word
        out.append(low.bit_length() - 1)
        word ^= low
    return out


class BrickModel(_Common):
    def __init__(self, hdr, cells, voxel_size, face_connected=False, box=None, inside_bricks=False, min_cells=1, stamp=0, seams=True,
                 wrap_mask=True):
        coord = brick_coords(hdr)
        occ = occ_of(np.asarray(cells, np.uint32).reshape(-1, 512))
        free, unk = layer_words(occ == 0), layer_words(occ == -1)
        place = {tuple(b): j for j, b in enumerate(coord.tolist())}       # the whole archive
        field = np.flatnonzero(in_box(coord, box))
        rank_of = {int(j): r for r, j in enumerate(field.tolist())}
        self.coords = coord[field]
        n = len(field)
        absent_reads = 0 if inside_bricks else ALL
        not0, not7 = (ALL & ~COL0, ALL & ~COL7) if wrap_mask else (ALL, ALL)
        border = (COL0, COL7, ROW0, ROW7, ALL, ALL)

        def masks(r, z):
            """per face the cells of layer z of field brick r whose neighbour across it reads unknown; the faces that look
            into an absent brick"""
            j = int(field[r])
            b = coord[j].tolist()
            nb = []
            for d in FACES:
                q = (b[0] + d[0], b[1] + d[1], b[2] + d[2])
                nb.append(place.get(q) if in_range(q) else None)
            w = [unk[k][z] if k is not None else absent_reads for k in nb[:4]]
            w.append(unk[j][z - 1] if z > 0 else unk[nb[4]][7] if nb[4] is not None else absent_reads)
            w.append(unk[j][z + 1] if z < 7 else unk[nb[5]][0] if nb[5] is not None else absent_reads)
            own = unk[j][z]
            m = [((own << 1) & not0 & ALL) | ((w[0] >> 7) & COL0), ((own >> 1) & not7) | ((w[1] << 7) & COL7),
                 ((own << 8) & ALL) | (w[2] >> 56), (own >> 8) | ((w[3] << 56) & ALL), w[4], w[5]]
            gone = [k is None for k in nb]
            gone[4], gone[5] = gone[4] and z == 0, gone[5] and z == 7
            return m, gone

        front = [[0] * 8 for _ in range(n)]
        pre = np.zeros(n * 8 + 1, np.int64)
        out_cells, out_faces, n_absent = [], [], 0
        for r in range(n):
            j = int(field[r])
            for z in range(8):
                m, gone = masks(r, z)
                fr = free[j][z]
                fw = fr & (m[0] | m[1] | m[2] | m[3] | m[4] | m[5])
                front[r][z] = fw
                pre[r * 8 + z + 1] = pre[r * 8 + z] + bin(fw).count("1")
                n_absent += sum(bin(fr & m[f] & border[f]).count("1") for f in range(6) if gone[f])
                for bit in bits_of(fw):
                    out_cells.append((coord[j][0] * 8 + (bit & 7), coord[j][1] * 8 + (bit >> 3), coord[j][2] * 8 + z))
                    out_faces.append(sum((m[f] >> bit) & 1 for f in range(6)))
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
            """the rank of cell (x, y, z) of field brick r, None if it is no frontier cell"""
            bit = x + 8 * y
            w = front[r][z]
            return int(pre[r * 8 + z]) + bin(w & ((1 << bit) - 1)).count("1") if (w >> bit) & 1 else None

        moves = [d for d in AROUND if not face_connected or sum(v != 0 for v in d) == 1]
        for r in range(n):                                   # inside a brick
            for z in range(8):
                for bit in bits_of(front[r][z]):
                    a = index_of(r, bit & 7, bit >> 3, z)
                    for d in moves:
                        x, y, zz = (bit & 7) + d[0], (bit >> 3) + d[1], z + d[2]
                        if 0 <= x < 8 and 0 <= y < 8 and 0 <= zz < 8:
                            o = index_of(r, x, y, zz)
                            if o is not None:
                                unite(a, o)
        if seams:                                            # across the seams, from the shell
            for r in range(n):
                b = self.coords[r].tolist()
                for z in range(8):
                    for bit in bits_of(front[r][z]):
                        lx, ly = bit & 7, bit >> 3
                        if not (lx in (0, 7) or ly in (0, 7) or z in (0, 7)):
                            continue
                        a = index_of(r, lx, ly, z)
                        for d in moves:
                            x, y, zz = lx + d[0], ly + d[1], z + d[2]
                            q = (b[0] + (x >> 3), b[1] + (y >> 3), b[2] + (zz >> 3))
                            if q == tuple(b) or not in_range(q):
                                continue
                            nr = rank_of.get(place.get(q, -1))
                            if nr is None or nr > r:
                                continue
                            o = index_of(nr, x & 7, y & 7, zz & 7)
                            if o is not None:
                                unite(a, o)
        label = [find(a) for a in range(total)]
        self._finish(n, out_cells, out_faces, label, n_absent, voxel_size, min_cells, flags_of(face_connected, box, inside_bricks), stamp)


class CellModel(_Common):
    def __init__(self, hdr, cells, voxel_size, face_connected=False, box=None, inside_bricks=False, min_cells=1, stamp=0):
        coord = brick_coords(hdr)
        words = np.asarray(cells, np.uint32).reshape(-1, 512)
        occ = occ_of(words)
        local = [(w & 7, (w >> 3) & 7, w >> 6) for w in range(512)]
        world = {}
        for j, b in enumerate(coord.tolist()):
            row = occ[j].tolist()
            for w, (cx, cy, cz) in enumerate(local):
                world[(b[0] * 8 + cx, b[1] * 8 + cy, b[2] * 8 + cz)] = row[w]
        field = np.flatnonzero(in_box(coord, box))
        self.coords = coord[field]
        out_cells, out_faces, n_absent = [], [], 0
        for j in field.tolist():
            b = coord[j].tolist()
            for w in np.flatnonzero(occ[j] == 0).tolist():
                c = (b[0] * 8 + local[w][0], b[1] * 8 + local[w][1], b[2] * 8 + local[w][2])
                unknown = absent = 0
                for d in FACES:
                    o = world.get((c[0] + d[0], c[1] + d[1], c[2] + d[2]))
                    if o is None and not inside_bricks:     # in no archived brick: never observed
                        absent += 1
                    elif o == -1:
                        unknown += 1
                if unknown + absent:
                    out_cells.append(c)
                    out_faces.append(unknown + absent)
                    n_absent += absent
        index = {c: i for i, c in enumerate(out_cells)}
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
                    if k is not None and label[k] < 0:
                        label[k] = i
                        todo.append(q)
        self._finish(len(field), out_cells, out_faces, label, n_absent, voxel_size, min_cells, flags_of(face_connected, box, inside_bricks), stamp)


def difference(got, want):
    """None, or what differs between two (cells, cluster, faces, table, info) answers - models or the library's getters"""
    names = ("cells", "cluster", "unknown_faces", "table", "info")
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
    return model.cells, model.cluster, model.faces, model.table, model.info
