"""The crafted archives of the world objects tests: hand-written bricks (WORLD_BRICK headers in brick order and 512 words
each), shared by tests/test_world_objects_ref.py (the two restatements against each other, no GPU) and
tests/test_world_objects_gpu.py (the library against them).  A case is a dict: hdr, cells and builds - a list of
(keywords of the build, what is known about its answer in closed form): `total` objects in all, `cells` counted cells,
`per_label` {label: objects}.  Every case feeds world_import on a fresh map of shape A."""
import itertools

import numpy as np

from tests.world_reach_cases import CFG, FREE, MM, UNKNOWN, bricks_of, from_grid, int16_edge  # noqa: F401

STATIC = 65535


def word(label, track=STATIC, occ=1):
    return np.uint32((occ & 0xFF) << 24 | label << 16 | track)


A1, B2, C3 = word(1), word(2), word(3)
BOTH = (dict(), dict(face_connected=True))


def case(hdr_cells, builds):
    return dict(hdr=hdr_cells[0], cells=hdr_cells[1], builds=builds)


def same(want, **kw):
    """the same closed form under both connectivities"""
    return [(dict(kw, **c), dict(want)) for c in BOTH]


def grid16():
    """2 x 2 x 2 bricks astride 0, never observed: cell c at index c + 8, [z, y, x]"""
    return np.full((16, 16, 16), UNKNOWN, np.uint32)


def put(g, c, w):
    g[c[2] + 8, c[1] + 8, c[0] + 8] = w


# ---- one cell; a full brick of one label, at (0, 0, 0) and at (-1, -1, -1) for negative sums
def one_cell():
    g = np.full((8, 8, 8), UNKNOWN, np.uint32)
    g[5, 2, 6] = A1
    return case(bricks_of({(3, -2, 1): g}), same(dict(total=1, cells=1)))


def full_brick(at):
    c = case(bricks_of({tuple(at): np.full((8, 8, 8), A1, np.uint32)}), same(dict(total=1, cells=512)))
    c["at"] = tuple(at)
    return c


def full_brick_closed_form(at):
    """-> n_cells, cell_min, cell_max, cell_sum, cell_sq of the one object: d = 0 .. 7 per axis from the first cell"""
    lo = np.array(at, np.int64) * 8
    return 512, lo, lo + 7, 512 * lo + 64 * 28, [64 * 140] * 3 + [8 * 28 * 28] * 3


# ---- a 3-D checkerboard of two labels by parity: every cell alone under 6-connectivity, two objects under 26
def checkerboard():
    z, y, x = np.indices((8, 8, 8))
    g = np.where((x + y + z) % 2 == 0, A1, B2).astype(np.uint32)
    return case(bricks_of({(0, 0, 0): g}), [(dict(), dict(total=2, cells=512, per_label={1: 1, 2: 1})),
                                            (dict(face_connected=True), dict(total=512, cells=512, per_label={1: 256, 2: 256}))])


# ---- the diagonal pair: two cells of one label that touch only along an edge (they differ in x and y) or at a corner,
# the cells between them empty (free), unknown, free but carrying the pair's label, or occupied by another label; inside a
# brick, or astride a face (x crosses), an edge (x and y cross) or the corner (all three cross) where the eight bricks meet
FILLERS = {"empty": FREE, "unknown": UNKNOWN, "free": word(1, occ=0), "other": B2}
PLACES = {"inside": (2, 2, 2), "face": (-1, 2, 2), "edge": (-1, -1, 2), "corner": (-1, -1, -1)}


def diagonal_pair(kind, filler, place):
    g = grid16()
    a = PLACES[place]
    span = (1, 1, 0) if kind == "edge" else (1, 1, 1)
    for d in itertools.product(*[range(s + 1) for s in span]):
        put(g, (a[0] + d[0], a[1] + d[1], a[2] + d[2]), FILLERS[filler])
    b = (a[0] + span[0], a[1] + span[1], a[2] + span[2])
    put(g, a, A1)
    put(g, b, A1)
    others = (4 - 2 if kind == "edge" else 8 - 2) if filler == "other" else 0     # the cells between are one object of label 2
    c = case(from_grid(g, (-1, -1, -1)), [(dict(), dict(total=1 + (1 if others else 0), cells=2 + others, per_label={1: 1})),
                                          (dict(face_connected=True), dict(cells=2 + others, per_label={1: 2}))])
    c["pair"] = (a, b)
    return c


# ---- the bridge: A (label 1), B (label 2), C (label 1) in a row along an axis - B carries nothing from A to C
def bridge(axis):
    g = grid16()
    for k, w in enumerate((A1, B2, A1)):
        c = [3, 3, 3]
        c[axis] = -2 + k        # -2, -1, 0: the row crosses the seam
        put(g, c, w)
    return case(from_grid(g, (-1, -1, -1)), same(dict(total=3, cells=3, per_label={1: 2, 2: 1})))


# ---- the x-wrap: (7, cy) and (0, cy + 1) are neighbours in the layer word (bits 7 + 8 cy and 8 + 8 cy), not in the brick
def x_wrap():
    g = np.full((8, 8, 8), UNKNOWN, np.uint32)
    g[4, 2, 7] = g[4, 3, 0] = A1
    g[1, 5, 7] = g[2, 6, 0] = A1        # the same a layer apart
    return case(bricks_of({(0, 0, 0): g}), same(dict(total=4, cells=4)))


# ---- seams: two cells in different bricks that touch across a face; the same with different labels; a box that leaves
# the second brick out; the second brick absent; bricks at the int16 edge beside those a key overflow would make neighbours
def seam_face(second=A1, skip=(), **kw):
    g = grid16()
    put(g, (-1, 3, 3), A1)
    put(g, (0, 3, 3), second)
    return from_grid(g, (-1, -1, -1), skip=skip), kw


def seam_cases():
    out = {}
    hc, _ = seam_face()
    out["seam face"] = case(hc, same(dict(total=1, cells=2)))
    hc, _ = seam_face(second=B2)
    out["seam other label"] = case(hc, same(dict(total=2, cells=2)))
    hc, _ = seam_face()
    out["seam box"] = case(hc, same(dict(total=1, cells=1), box=((-1, -1, -1), (-1, 0, 0))))
    hc, _ = seam_face(skip=[(0, 0, 0)])
    out["seam absent"] = case(hc, same(dict(total=1, cells=1)))
    e = int16_edge()
    out["int16 edge"] = case((e["hdr"], np.where(e["cells"] == FREE, A1, e["cells"]).astype(np.uint32)), same(dict(total=len(e["hdr"]), cells=512 * len(e["hdr"]))))
    return out


# ---- a serpentine of label 1 confined to one brick, label 2 round it: rows along x at even y joined at alternating ends,
# on the even layers, one cell on the odd layers between them - 143 cells in a row, the first of them the brick's cell 0:
# its label needs 142 sweeps to arrive at the other end
def serpentine_brick():
    g = np.full((8, 8, 8), B2, np.uint32)
    at = [0, 0]                      # where the snake stands: x end, y
    for z in range(0, 8, 2):
        ys = range(0, 8, 2) if at[1] == 0 else range(6, -1, -2)
        for k, y in enumerate(ys):
            g[z, y, :] = A1
            at[0] = 7 - at[0]
            if k < 3:
                g[z, y + (1 if at[1] == 0 else -1), at[0]] = A1
        at[1] = 6 - at[1]
        if z < 6:
            g[z + 1, at[1], at[0]] = A1
    n = int((g == A1).sum())
    assert n == 4 * 35 + 3
    return case(bricks_of({(0, 0, 0): g}), [(dict(face_connected=True), dict(cells=512, per_label={1: 1}))] + [(dict(), dict(cells=512, per_label={1: 1}))])


# ---- a one-cell-wide tube of label 1 snaking through 2 x 3 x 5 = 30 bricks, and round it, against it all the way, a
# sheath of label 2: two objects
def serpentine_tube():
    g = np.full((16, 24, 40), UNKNOWN, np.uint32)
    t = np.zeros(g.shape, bool)
    rows = list(range(2, 24, 4))
    for level, z in enumerate((3, 11)):
        ys = rows if level == 0 else rows[::-1]
        for k, y in enumerate(ys):
            t[z, y, 1:39] = True
            if k + 1 < len(ys):
                x = 38 if k % 2 == 0 else 1
                t[z, min(y, ys[k + 1]):max(y, ys[k + 1]) + 1, x] = True
    t[3:12, rows[-1], 38 if (len(rows) - 1) % 2 == 0 else 1] = True
    near = np.zeros(g.shape, bool)
    for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3):
        near[max(dz, 0):16 + min(dz, 0), max(dy, 0):24 + min(dy, 0), max(dx, 0):40 + min(dx, 0)] |= \
            t[max(-dz, 0):16 + min(-dz, 0), max(-dy, 0):24 + min(-dy, 0), max(-dx, 0):40 + min(-dx, 0)]
    g[near] = B2
    g[t] = A1
    return case(from_grid(g, (-2, -1, -1)), same(dict(total=2, cells=int(near.sum()), per_label={1: 1, 2: 1})))


# ---- more bricks than a scan tile of 2048: a plate of 46 x 46 bricks, in each the row cy = 3 and the column cx = 3 of the
# layer cz = 3 - one lattice, one object
def plate():
    n = 46
    g = np.full((8, 8 * n, 8 * n), UNKNOWN, np.uint32)
    g[3, 3::8, :] = A1
    g[3, :, 3::8] = A1
    return case(from_grid(g, (-20, -23, 4)), same(dict(total=1, cells=n * n * 15)))


# ---- BY_TRACK: one label on two touching tracks
def two_tracks():
    g = np.full((8, 8, 8), UNKNOWN, np.uint32)
    g[2, 2, 1:4] = word(1, track=2)
    g[2, 2, 4:7] = word(1, track=STATIC)
    c = case(bricks_of({(0, 0, 0): g}), same(dict(total=1, cells=6)) + same(dict(total=2, cells=6), by_track=True))
    return c


# ---- every filter flag: static, movable (track 3 <= max_movable_track), guessed (occ 2) words; the label mask
def filters():
    g = np.full((8, 8, 8), UNKNOWN, np.uint32)
    g[0, 0, 0:2] = word(1)                      # static, observed
    g[0, 2, 0:3] = word(1, track=3)             # movable
    g[0, 4, 0:4] = word(2, occ=2)               # static, guessed
    g[0, 6, 0:5] = word(3, track=3, occ=2)      # movable, guessed
    g[7, 7, 7] = word(1, occ=0)                 # free: never counted
    builds = []
    for kw, cells, total in ((dict(), 14, 4), (dict(static_only=True), 6, 2), (dict(movable_only=True), 8, 2), (dict(observed_only=True), 5, 2),
                             (dict(static_only=True, observed_only=True), 2, 1), (dict(movable_only=True, observed_only=True), 3, 1),
                             (dict(labels=(1,)), 5, 2), (dict(labels=(2, 3, 200)), 9, 2), (dict(labels=()), 0, 0),
                             (dict(min_cells=3), 14, 4), (dict(min_cells=6), 14, 4)):
        builds += same(dict(total=total, cells=cells), **kw)
    return case(bricks_of({(1, 1, 1): g}), builds)


# ---- empty fields: an empty box; a brick without a counted cell
def empty_fields():
    g = np.full((8, 8, 8), FREE, np.uint32)
    return case(bricks_of({(0, 0, 0): g}), same(dict(total=0, cells=0)) + same(dict(total=0, cells=0), box=((0, 0, 0), (0, -1, 0))) +
                same(dict(total=0, cells=0), box=((5, 5, 5), (6, 6, 6))))


# ---- random: 4 x 4 x 2 bricks, three missing, three labels at about 30 % density, movable and guessed words among them
RANDOM_SKIP = [(0, 1, 0), (2, 2, 1), (-1, 0, 1)]
RANDOM_BOX = ((0, -1, 0), (2, 1, 1))


def random_archive(seed=31):
    rng = np.random.default_rng(seed)
    u = rng.random((16, 32, 32))
    g = np.full(u.shape, FREE, np.uint32)
    g[u > 0.85] = UNKNOWN
    g[u < 0.30] = C3
    g[u < 0.20] = B2
    g[u < 0.10] = A1
    v = rng.random(u.shape)
    occupied = u < 0.30
    g[occupied & (v < 0.15)] = (g[occupied & (v < 0.15)] & np.uint32(0xFFFF0000)) | np.uint32(3)              # movable
    g[occupied & (v > 0.9)] = (g[occupied & (v > 0.9)] & np.uint32(0x00FFFFFF)) | np.uint32(2 << 24)           # guessed
    return from_grid(g, (-1, -1, 0), skip=RANDOM_SKIP)


def random_variants():
    """16 option sets and a box"""
    out = [dict(face_connected=f, by_track=t, static_only=s, min_cells=m)
           for f, t, s, m in itertools.product((False, True), (False, True), (False, True), (1, 3))]
    out.append(dict(box=RANDOM_BOX, observed_only=True, labels=(1, 3)))
    return out


def crafted():
    """name -> case"""
    out = {"one cell": one_cell(), "full brick": full_brick((0, 0, 0)), "full brick at -1": full_brick((-1, -1, -1)),
           "checkerboard": checkerboard(), "x wrap": x_wrap(), "serpentine brick": serpentine_brick(), "serpentine tube": serpentine_tube(),
           "plate": plate(), "two tracks": two_tracks(), "filters": filters(), "empty fields": empty_fields()}
    for kind, filler, place in itertools.product(("edge", "corner"), FILLERS, PLACES):
        if kind == "edge" and place == "corner":
            continue                     # (an edge pair crosses two seams at the most)
        out["pair %s %s %s" % (kind, filler, place)] = diagonal_pair(kind, filler, place)
    for axis in range(3):
        out["bridge %s" % "xyz"[axis]] = bridge(axis)
    out.update(seam_cases())
    return out


def check_closed_forms(name, c, k, ref):
    """build k of case c against what is known of it without any model"""
    want = c["builds"][k][1]
    if "total" in want:
        assert ref.info["n_objects_total"] == want["total"], (name, k, ref.info["n_objects_total"], want)
    if "cells" in want:
        assert ref.info["n_cells"] == want["cells"], (name, k, ref.info["n_cells"], want)
    for label, count in want.get("per_label", {}).items():
        assert ref.label_objects[label] == count, (name, k, label, ref.label_objects[label], want)
    if name.startswith("full brick") and len(ref.table):
        n, lo, hi, total, sq = full_brick_closed_form(c["at"])
        e = ref.table[0]
        assert e["n_cells"] == n and e["cell_min"].tolist() == lo.tolist() and e["cell_max"].tolist() == hi.tolist()
        assert e["cell_sum"].tolist() == total.tolist() and e["cell_sq"].tolist() == sq and e["first_cell"].tolist() == lo.tolist()
        size = np.float32(CFG["voxel_size"])
        assert e["box_min"].tolist() == (lo.astype(np.float32) * size).tolist() and e["box_max"].tolist() == ((hi + 1).astype(np.float32) * size).tolist()
        assert np.allclose(e["centroid"], (lo + 4.0) * float(size), rtol=1e-6, atol=0)
    if name == "two tracks" and len(ref.table):
        assert [int(v) for v in ref.table["mixed_tracks"]] == ([0, 0] if c["builds"][k][0].get("by_track") else [1])
