"""The crafted archives of the world distance field tests: hand-written bricks (WORLD_BRICK headers in brick order and 512
words each), shared by tests/test_world_esdf_ref.py (the two restatements against each other, no GPU) and
tests/test_world_esdf_gpu.py (the library against them).  A case is a dict: hdr, cells and kw, the build's keywords
(radius among them); some carry what the tests assert beyond equality.  Every case feeds world_import on a fresh map of
shape A.  Each is the smallest archive that shows one way to go wrong."""
import itertools

import numpy as np

from tests.world_reach_cases import CFG, FREE, MM, MOVING, UNKNOWN, WALL, ball, bricks_of, from_grid, int16_edge, pillars, random_world  # noqa: F401

NONE = 0xFFFF


def case(hdr_cells, radius, **kw):
    return dict(hdr=hdr_cells[0], cells=hdr_cells[1], kw=dict(kw, radius=radius))


def word_of(c):
    """world cell -> (brick, cell word)"""
    return (c[0] >> 3, c[1] >> 3, c[2] >> 3), (c[0] & 7) | (c[1] & 7) << 3 | (c[2] & 7) << 6


# 1 ---- the ball: one obstacle at world cell (0, 0, 0), where eight bricks meet (seven with skip: brick (-1, -1, -1))
def ball_case(radius, skip=False, **kw):
    b = ball(0, skip)
    c = case((b["hdr"], b["cells"]), radius, **kw)
    c["obstacle"], c["skipped"] = (0, 0, 0), (-1, -1, -1) if skip else None
    return c


# 2 ---- x-wrap: an obstacle at (cx 7, cy 2) and a free cell at (cx 0, cy 3) are neighbours in the layer word (bits 23 and
# 24), not in space: d2 is 7^2 + 1 = 50, not 1
def x_wrap():
    g = np.full((8, 8, 8), FREE, np.uint32)
    g[4, 2, 7] = WALL
    c = case(bricks_of({(0, 0, 0): g}), 8)
    c["probe"], c["want"] = (0, 3, 4), (50, (7, -1, 0))
    return c


# 3 ---- far reach: five bricks in a row along `axis`, -2 .. 2; obstacles as a list of world cells
def row_of_five(axis, obstacles, radius, skip=()):
    shape = [8, 8, 8]
    shape[2 - axis] = 40
    g = np.full(shape, FREE, np.uint32)            # [z, y, x]; the cell at -16 along the axis is index 0
    for q in obstacles:
        i = [q[2], q[1], q[0]]
        i[2 - axis] += 16
        g[tuple(i)] = WALL
    lo = [0, 0, 0]
    lo[axis] = -2
    sk = []
    for s in skip:
        b = [0, 0, 0]
        b[axis] = s
        sk.append(tuple(b))
    return case(from_grid(g, tuple(lo), skip=sk), radius)


def along(axis, v, other=(3, 3)):
    c = [other[0], other[1]]
    c.insert(axis, v)
    return tuple(c)


def far_reach(axis, radius):
    """`probes`: (world cell, d2 or NONE) pairs"""
    if radius == 8:
        # the obstacle at 8 along the axis, in brick 1: the cell at 0 (brick 0, across one seam) is 8 away, the one at -1 is 9
        c = row_of_five(axis, [along(axis, 8)], 8)
        c["probes"] = [(along(axis, 0), 64), (along(axis, -1), NONE), (along(axis, 15), 49), (along(axis, 16), 64), (along(axis, 17), NONE)]
    else:
        # at cx 0 of brick -2 and at cx 7 of brick +2: cell 0 of brick 0 is 16 from the first, cell 7 16 from the second
        c = row_of_five(axis, [along(axis, -16), along(axis, 23)], 16)
        c["probes"] = [(along(axis, 0), 256), (along(axis, 7), 256), (along(axis, 1), NONE), (along(axis, 6), NONE), (along(axis, -1), 225),
                       (along(axis, 8), 225)]
    return c


def far_diagonal():
    """a 5 x 5 x 1 plate of bricks, an obstacle at offset (-12, -10, 0) of the cell (0, 0, 3), in brick (-2, -2, 0): 244"""
    g = np.full((8, 40, 40), FREE, np.uint32)
    g[3, 16 - 10, 16 - 12] = WALL
    c = case(from_grid(g, (-2, -2, 0)), 16)
    c["probes"] = [((0, 0, 3), 244), ((1, 0, 3), NONE), ((0, 2, 3), NONE), ((0, 1, 3), NONE)]   # 269, 288, 265
    return c


# 4 ---- absent between: the brick between the cell and the obstacle is not archived; the obstacle still counts
def absent_between(axis):
    c = row_of_five(axis, [along(axis, 12)], 16, skip=(0, 2, -2))    # bricks -1 and 1 remain; the obstacle in brick 1
    c["probes"] = [(along(axis, -1), 169), (along(axis, -4), 256), (along(axis, -5), NONE)]
    c["n_bricks"] = 2
    return c


# 5 ---- ties
def ties(kind):
    g = np.full((8, 8, 8), FREE, np.uint32)
    if kind in ("x", "y", "z"):                    # midway between two walls along the axis
        axis = "xyz".index(kind)
        for v in (1, 7):
            s = [slice(None)] * 3
            s[2 - axis] = v
            g[tuple(s)] = WALL
        want = [0, 0, 0]
        want[axis] = -3
        c = case(bricks_of({(0, 0, 0): g}), 8)
        c["probe"], c["want"] = along(axis, 4, (4, 4)), (9, tuple(want))
    else:                                          # obstacles at (-3, 0, 0), (0, 0, -3) and (0, 3, 0) of the cell (4, 4, 4)
        g[4, 4, 1] = g[1, 4, 4] = g[4, 7, 4] = WALL
        c = case(bricks_of({(0, 0, 0): g}), 8)
        c["probe"], c["want"] = (4, 4, 4), (9, (0, 0, -3))   # the smallest world cell in (z, y, x) order: the one below
    return c


# 6 ---- box: a field of one brick whose nearest wall is in the brick outside the box
def box_case():
    g = np.full((8, 8, 16), FREE, np.uint32)
    g[:, :, 10] = WALL                              # the plane x = 10, in brick (1, 0, 0)
    c = case(from_grid(g), 8, box=((0, 0, 0), (0, 0, 0)))
    c["probes"] = [((7, 2, 2), 9), ((2, 5, 1), 64), ((1, 5, 1), NONE)]
    c["n_bricks"] = 1
    return c


# 7 ---- the int16 edge
def edge_case(unknown_is_obstacle, radius=3):
    e = int16_edge()
    return case((e["hdr"], e["cells"]), radius, unknown_is_obstacle=unknown_is_obstacle)


# 8 ---- pillars with moving obstacles
def pillars_case(static_only, radius=8):
    p = pillars(0, False)
    return case((p["hdr"], p["cells"]), radius, static_only=static_only)


# 9 ---- random: 5 x 5 x 5 bricks round (0, 0, 0) without two corners and an edge: a shell three cells thick of random
# words round a free cavity, some unknown cells and movable obstacles inside it but more than 17 cells from the middle.  The
# cavity's middle cells are more than 16 cells from everything, under every flag: NONE, 0 and values in between occur in
# every build below.
RANDOM_SKIP = [(-2, -2, -2), (2, 2, 0), (2, -2, 2)]
RANDOM_BOX = ((-2, -1, 0), (0, 1, 1))
RANDOM_RADII = (1, 3, 8, 9, 16)


def random_archive(seed=31):
    rng = np.random.default_rng(seed)
    u = rng.random((40, 40, 40))
    g = np.full(u.shape, FREE, np.uint32)
    i = np.arange(40)
    shell = (i < 3) | (i > 36)
    in_shell = shell[:, None, None] | shell[None, :, None] | shell[None, None, :]
    g[in_shell & (u < 0.4)] = UNKNOWN
    g[in_shell & (u < 0.3)] = WALL
    g[in_shell & (u < 0.1)] = MOVING
    for z, y, x, w in ((20, 6, 6, UNKNOWN), (12, 10, 33, UNKNOWN), (30, 31, 9, UNKNOWN), (20, 30, 5, MOVING), (8, 8, 30, MOVING), (32, 31, 10, WALL),
                       (6, 30, 8, WALL), (22, 36, 8, UNKNOWN)):
        g[z, y, x] = w
    return from_grid(g, (-2, -2, -2), skip=RANDOM_SKIP)


def random_variants():
    return [dict(radius=r, unknown_is_obstacle=u, static_only=s, box=b)
            for u, s, b, r in itertools.product((False, True), (False, True), (None, RANDOM_BOX), RANDOM_RADII)]


def crafted():
    """name -> case"""
    out = {"x wrap": x_wrap(), "far diagonal": far_diagonal(), "box": box_case()}
    for r in (1, 2, 3, 8, 9, 16):
        out["ball R=%d" % r] = ball_case(r)
    for r in (2, 9, 16):
        out["ball skip R=%d" % r] = ball_case(r, skip=True)
        out["ball skip solid R=%d" % r] = ball_case(r, skip=True, unknown_is_obstacle=True)
    for axis in range(3):
        out["far 8 %s" % "xyz"[axis]] = far_reach(axis, 8)
        out["far 16 %s" % "xyz"[axis]] = far_reach(axis, 16)
        out["absent between %s" % "xyz"[axis]] = absent_between(axis)
    for kind in ("x", "y", "z", "three"):
        out["ties " + kind] = ties(kind)
    for u in (False, True):
        out["int16 edge solid=%s" % u] = edge_case(u)
    for s in (False, True):
        out["pillars static_only=%s" % s] = pillars_case(s)
    return out
