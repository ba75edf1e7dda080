"""NumPy restatement of the frontiers (include/sdm.h: sdm_frontiers_update / sdm_get_frontier_clusters /
sdm_get_frontier_cells), for the tests.  No SciPy.

Takes what a caller can read back from a map - voxels(), ring_state() through tests/query_ref.Geometry, and the
configuration - or an occ block indexed [z, y, x] directly.  The frontier mask comes from shifted arrays; the labels from
the sorted sparse cell list: every cell looks its preceding neighbours up with np.searchsorted, and the edges found are
worked off by min-hooking and pointer jumping until nothing changes (logarithmically many rounds, so a long snake on a
2 M-voxel map stays fast); the table from integer reductions per root and the header's float formulas, one operation at
a time.
"""
import numpy as np

from semantic_dsp_map_amd.binding import FRONTIER_CLUSTER, FRONTIER_NO_CLUSTER

# (dz, dy, dx) of the neighbours that precede a cell in cell order
PRECEDING_26 = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) < (0, 0, 0)]
PRECEDING_6 = [o for o in PRECEDING_26 if sum(map(abs, o)) == 1]
assert len(PRECEDING_26) == 13 and len(PRECEDING_6) == 3


def occ_grid(geo, voxels):
    """occ indexed [z, y, x] in map-index cells"""
    return voxels["occ"][geo.voxel_grid()]


def origin_of(geo):
    return (geo.center + geo.pmin).astype(np.float32)


def frontier_mask(occ):
    """-> (mask, faces): bool and uint8 arrays [z, y, x]; faces = unknown face neighbours inside the block of every cell"""
    unknown = occ == -1
    faces = np.zeros(occ.shape, np.uint8)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(None, -1), slice(1, None)
        faces[tuple(hi)] += unknown[tuple(lo)]   # the neighbour below on this axis
        faces[tuple(lo)] += unknown[tuple(hi)]   # ... and above
    return (occ == 0) & (faces > 0), faces


def label_cells(cells, shape, face_connected):
    """cells: ascending cell words of a block [NZ, NY, NX] -> per cell the position (rank) of its component's smallest cell"""
    NZ, NY, NX = (int(n) for n in shape)
    cells = np.asarray(cells, np.int64)
    n = len(cells)
    parent = np.arange(n, dtype=np.int64)
    if n == 0:
        return parent
    x, y, z = cells % NX, (cells // NX) % NY, cells // (NX * NY)
    ea, eb = [], []
    for dz, dy, dx in (PRECEDING_6 if face_connected else PRECEDING_26):
        nx, ny, nz = x + dx, y + dy, z + dz
        ok = (nx >= 0) & (nx < NX) & (ny >= 0) & (ny < NY) & (nz >= 0) & (nz < NZ)
        word = nx + NX * (ny + NY * nz)
        pos = np.minimum(np.searchsorted(cells, word), n - 1)
        ok &= cells[pos] == word
        ea.append(np.flatnonzero(ok))
        eb.append(pos[ok])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    while True:
        pa, pb = parent[ea], parent[eb]
        open_ = pa != pb
        if not open_.any():
            return parent
        ea, eb, pa, pb = ea[open_], eb[open_], pa[open_], pb[open_]
        lo = np.minimum(pa, pb)
        np.minimum.at(parent, pa, lo)   # min-hooking: a root gets the smallest root it has an edge to
        np.minimum.at(parent, pb, lo)
        while True:                      # pointer jumping until every cell points at a root
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt


def frontiers_of_block(occ, origin, voxel_size, face_connected=False, min_cells=1):
    """occ [z, y, x] -> dict(table, cell, cluster, unknown_faces) as the getters must return them"""
    NZ, NY, NX = occ.shape
    mask, faces = frontier_mask(occ)
    cell = np.flatnonzero(mask.ravel())   # [z, y, x] row-major = i | j << x_n | k << (x_n + y_n), ascending
    root = label_cells(cell, occ.shape, face_connected)
    fc = faces.ravel()[cell]
    roots, inv, counts = np.unique(root, return_inverse=True, return_counts=True)
    keep = counts >= max(int(min_cells), 1)
    index = np.full(len(roots), FRONTIER_NO_CLUSTER, np.int64)
    index[keep] = np.arange(int(keep.sum()))
    out = dict(cell=cell.astype(np.uint32), cluster=index[inv].astype(np.uint32) if len(cell) else np.zeros(0, np.uint32),
               unknown_faces=fc.astype(np.uint8))
    table = np.zeros(int(keep.sum()), FRONTIER_CLUSTER)
    out["table"] = table
    if not len(table):
        return out
    c = cell.astype(np.int64)
    ijk = [c % NX, (c // NX) % NY, c // (NX * NY)]
    k = len(roots)
    table["first_cell"] = cell[roots][keep]
    table["first_index"] = roots[keep]
    table["n_cells"] = counts[keep]
    nf = np.zeros(k, np.int64)
    np.add.at(nf, inv, fc.astype(np.int64))
    table["n_unknown_faces"] = nf[keep]
    size = np.float32(voxel_size)
    origin = np.asarray(origin, np.float32)
    for a in range(3):
        lo, hi, s = np.full(k, 1 << 20, np.int64), np.full(k, -1, np.int64), np.zeros(k, np.int64)
        np.minimum.at(lo, inv, ijk[a])
        np.maximum.at(hi, inv, ijk[a])
        np.add.at(s, inv, ijk[a])
        lo, hi, s = lo[keep], hi[keep], s[keep]
        table["cell_min"][:, a], table["cell_max"][:, a], table["cell_sum"][:, a] = lo, hi, s
        table["box_min"][:, a] = origin[a] + lo.astype(np.float32) * size
        table["box_max"][:, a] = origin[a] + (hi + 1).astype(np.float32) * size
        mean = s.astype(np.float64) / counts[keep].astype(np.float64)
        table["centroid"][:, a] = (np.float64(origin[a]) + (mean + np.float64(0.5)) * np.float64(size)).astype(np.float32)
    return out


def frontiers(geo, voxels, voxel_size, face_connected=False, min_cells=1):
    return frontiers_of_block(occ_grid(geo, voxels), origin_of(geo), voxel_size, face_connected, min_cells)


def storage_coords(geo, cell):
    """(n, 3) storage (ring) coordinates of map-index cell words"""
    c = np.asarray(cell, np.int64)
    x_n, y_n = int(geo.n_bits[0]), int(geo.n_bits[1])
    m = np.stack([c & ((1 << x_n) - 1), (c >> x_n) & ((1 << y_n) - 1), c >> (x_n + y_n)], axis=1)
    r = m + geo.eq
    return np.where(r < 0, r + geo.N, np.where(r >= geo.N, r - geo.N, r))


def equal_tables(a, b):
    """None if the two tables are equal on every field of every entry, floats by their bit patterns; else what differs"""
    if len(a) != len(b):
        return "length %d != %d (first cells %s / %s)" % (len(a), len(b), a["first_cell"][:12], b["first_cell"][:12])
    for k in FRONTIER_CLUSTER.names:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            bad = np.flatnonzero((x != y).reshape(len(a), -1).any(axis=1))
            return "%s differs at entries %s: %s / %s" % (k, bad[:5], a[k][bad[:3]], b[k][bad[:3]])
    return None


def equal_all(got_table, got_cells, ref):
    """the table and the three per-cell arrays (cell, cluster, unknown_faces) against frontiers()'s dict"""
    for k, g in zip(("cell", "cluster", "unknown_faces"), got_cells):
        if not np.array_equal(g, ref[k]):
            if len(g) != len(ref[k]):
                return "%s: %d cells != %d" % (k, len(g), len(ref[k]))
            bad = np.flatnonzero(g != ref[k])
            return "%s differs at cells %s: %s / %s" % (k, bad[:5], g[bad[:5]], ref[k][bad[:5]])
    return equal_tables(got_table, ref["table"])
