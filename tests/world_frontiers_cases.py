"""The crafted archives of the world frontier tests: hand-written bricks (WORLD_BRICK headers in brick order and 512 words
each), shared by tests/test_world_frontiers_ref.py (the two restatements against each other, no GPU) and
tests/test_world_frontiers_gpu.py (the library against them).  A case is a dict: hdr, cells and kw, the build's keywords;
some carry what the tests assert beyond equality.  Every case feeds world_import on a fresh map of shape A."""
import itertools

import numpy as np

from tests.world_reach_cases import CFG, FREE, UNKNOWN, WALL, bricks_of, from_grid, int16_edge, plate, random_world  # noqa: F401


def case(hdr_cells, **kw):
    return dict(hdr=hdr_cells[0], cells=hdr_cells[1], kw=kw)


# 1 ---- one brick, all free, alone: its shell is the frontier, 296 cells with 1 (face), 2 (edge) or 3 (corner) faces
def one_free(at=(0, 0, 0), **kw):
    c = case(bricks_of({tuple(at): np.full((8, 8, 8), FREE, np.uint32)}), **kw)
    c["at"] = tuple(at)
    return c


# 2 ---- one free brick with one unknown cell in the middle
def hole(**kw):
    g = np.full((8, 8, 8), FREE, np.uint32)
    g[4, 4, 4] = UNKNOWN
    return case(bricks_of({(2, -1, 0): g}), inside_bricks=True, **kw)


# 3 ---- x-wrap: unknown at (cx 0, cy 3) and free at (cx 7, cy 2) are neighbours in the layer word (bits 24 and 23), not in
# the brick; so are unknown at (7, 5) and free at (0, 6) (bits 47 and 48).  Everything else is a wall: no frontier cell.
def x_wrap():
    g = np.full((8, 8, 8), WALL, np.uint32)
    g[2, 3, 0], g[2, 2, 7] = UNKNOWN, FREE
    g[5, 5, 7], g[5, 6, 0] = UNKNOWN, FREE
    return case(bricks_of({(0, 0, 0): g}), inside_bricks=True)


# 4 ---- seams: 2 x 2 x 2 bricks astride 0, walls but for two free cells in different bricks, each with an unknown cell
# behind it, that touch only across a face, an edge or the corner
def seams(kind, **kw):
    g = np.full((16, 16, 16), WALL, np.uint32)   # cell c at index c + 8, [z, y, x]
    a, b = {"face": ((-1, 3, 3), (0, 3, 3)), "edge": ((-1, -1, 3), (0, 0, 3)), "corner": ((-1, -1, -1), (0, 0, 0))}[kind]
    for c, behind in ((a, -1), (b, 1)):
        g[c[2] + 8, c[1] + 8, c[0] + 8] = FREE
        g[c[2] + 8, c[1] + 8, c[0] + 8 + behind] = UNKNOWN
    out = case(from_grid(g, (-1, -1, -1)), inside_bricks=True, **kw)
    out["pair"] = (a, b)
    return out


# 5 / 6 ---- two free bricks side by side and a third missing; the same archive with a box of one brick
def absent_neighbour(**kw):
    free = np.full((8, 8, 8), FREE, np.uint32)
    return case(bricks_of({(0, 0, 0): free, (1, 0, 0): free}), **kw)


# 7 ---- a one-cell-wide unknown tube snaking through 2 x 3 x 5 = 30 bricks of free space: rows along x every four cells
# of y on two levels of z, joined at alternating ends; the free cells round it are one cluster (26-connected) whose union
# tree is deep and crosses faces, edges and corners of bricks
def serpentine(**kw):
    g = np.full((16, 24, 40), FREE, np.uint32)
    rows = list(range(2, 24, 4))
    for level, z in enumerate((3, 11)):
        ys = rows if level == 0 else rows[::-1]
        for k, y in enumerate(ys):
            g[z, y, 1:39] = UNKNOWN
            if k + 1 < len(ys):
                x = 38 if k % 2 == 0 else 1      # (both levels enter their first row at x = 1)
                g[z, min(y, ys[k + 1]):max(y, ys[k + 1]) + 1, x] = UNKNOWN
    g[3:12, rows[-1], 38 if (len(rows) - 1) % 2 == 0 else 1] = UNKNOWN   # up from the end of the first level
    return case(from_grid(g, (-2, -1, -1)), inside_bricks=True, **kw)


# 10 ---- random: the random archive of the world reach tests, about 5 % of its free cells turned unknown
def random_archive(seed=23):
    hdr, cells = random_world()
    rng = np.random.default_rng(seed)
    cells = cells.copy()
    cells[(cells == FREE) & (rng.random(cells.shape) < 0.05)] = UNKNOWN
    return hdr, cells


RANDOM_BOX = ((0, -1, 0), (2, 1, 1))


def random_variants():
    return [dict(face_connected=f, inside_bricks=i, box=b, min_cells=m)
            for f, i, b, m in itertools.product((False, True), (False, True), (None, RANDOM_BOX), (1, 4))]


def crafted():
    """name -> case"""
    out = {"one free": one_free(), "one free inside": one_free(inside_bricks=True), "one free at -1": one_free((-1, -1, -1)),
           "hole": hole(), "hole face": hole(face_connected=True), "x wrap": x_wrap(),
           "absent neighbour": absent_neighbour(), "box": absent_neighbour(box=((0, 0, 0), (0, 0, 0))),
           "serpentine": serpentine(), "serpentine face": serpentine(face_connected=True),
           "plate": case((plate(False)["hdr"], plate(False)["cells"])), "int16 edge": case((int16_edge()["hdr"], int16_edge()["cells"]))}
    for kind in ("face", "edge", "corner"):
        out["seams " + kind] = seams(kind)
        out["seams %s face" % kind] = seams(kind, face_connected=True)
    return out
