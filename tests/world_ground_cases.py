"""The crafted archives of the world ground tests: hand-written bricks (WORLD_BRICK headers in brick order and 512 words
each), shared by tests/test_world_ground_ref.py (the two restatements against each other and against the values written
here, no GPU) and tests/test_world_ground_gpu.py (the library against them).  A case is a dict: hdr, cells, kw - the build's
keywords - and `expect`, a function of a model that asserts what was worked out by hand.  World cells are (x, y, z); the
default orientation is z up, so a column is (x, y) and a height is z."""
import itertools

import numpy as np

from semantic_dsp_map_amd.binding import FOOTPRINT
from tests.world_reach_cases import CFG, FREE, MM, MOVING, UNKNOWN, WALL, bricks_of, from_grid, int16_edge, random_world

NO = 0xFFFF
NONE = 0xFFFF
FLOOR = WALL                              # label 8, a static track
KERB = 1 << 24 | 9 << 16 | 65535          # occupied, static, a label outside the masks used here
HIGH = 1 << 24 | 40 << 16 | 65535         # occupied, static, a label in the mask's second word
SUPPORT = [8]
assert (WALL >> 16) & 0xFF == 8 and (MOVING >> 16) & 0xFF == 7 and 1 <= (MOVING & 0xFFFF) <= MM < 65535


def case(hdr_cells, expect=None, **kw):
    kw.setdefault("support_labels", SUPPORT)
    return dict(hdr=hdr_cells[0], cells=hdr_cells[1], kw=kw, expect=expect)


def column(m, i, j):
    """(cell record, d2) of world column (i, j) of a model or of a library answer wrapped as one"""
    r = m.rank[(i >> 3, j >> 3)]
    w = (i & 7) | (j & 7) << 3
    return m.cells[r, w], int(m.d2[r, w])


def fields(c):
    return tuple(int(c[f]) for f in ("level", "top", "label", "cls", "headroom", "n_unknown"))


# 1 ---- every orientation: one brick, a floor layer at cell 3 of the up axis with a free layer over it, the rest unknown
def orientation(axis, sign, at):
    g = np.full((8, 8, 8), UNKNOWN, np.uint32)           # [cz, cy, cx]
    sl = [slice(None)] * 3
    sl[2 - axis] = 3
    g[tuple(sl)] = FLOOR
    sl[2 - axis] = 3 + sign
    g[tuple(sl)] = FREE
    b = [0, 0, 0]
    b[axis] = at
    h_lo = 8 * at if sign > 0 else -1 - (8 * at + 7)
    level = 3 if sign > 0 else 4

    def expect(m):
        assert m.coords.tolist() == [[0, 0]] and m.info["n_ground"] == 64 and m.info["n_lethal"] == 0
        # 7 - level unknown cells above the floor's free layer ... and `level` below it
        assert all(fields(c) == (level, level, 8, 1, 1, 6) for c in m.cells[0]), m.cells[0][0]
        assert (m.d2 == NONE).all() and m.info["level_min"] == m.info["level_max"] == level

    return case(bricks_of({tuple(b): g}), expect, up=(axis, sign), h_lo=h_lo, h_hi=h_lo + 7, clearance=1, radius=8)


# 2 ---- height seams
def seam(above, blocker=None):
    """a floor at z = 7 of brick (0, 0, 0); `above`: the bricks over it that exist, all free; blocker: a wall cell at that z"""
    words = {(0, 0, 0): np.full((8, 8, 8), UNKNOWN, np.uint32)}
    words[(0, 0, 0)][7] = FLOOR
    for bz in above:
        words[(0, 0, bz)] = np.full((8, 8, 8), FREE, np.uint32)
    if blocker is not None:
        words[(0, 0, blocker >> 3)][blocker & 7] = KERB
    return bricks_of(words)


def seams():
    out = {}

    def level7(headroom):
        def expect(m):
            assert all(fields(c) == (7, 7, 8, 1, headroom, 7) for c in m.cells[0]), m.cells[0][0]
        return expect

    def obstacle(m):
        assert all(fields(c) == (NO, 7, 0, 2 | 8, 0, 7) for c in m.cells[0]), m.cells[0][0]
        assert (m.d2 == 0).all()

    band = dict(h_lo=0, h_hi=7, radius=4)
    out["seam clearance in the brick above"] = case(seam([1]), level7(2), clearance=2, **band)
    out["seam brick above absent"] = case(seam([]), obstacle, clearance=2, **band)
    out["seam brick above absent, unknown passable"] = case(seam([]), level7(2), clearance=2, unknown_passable=True, **band)
    out["seam clearance over two bricks"] = case(seam([1, 2]), level7(12), clearance=12, **band)
    out["seam blocker at h_hi + clearance"] = case(seam([1, 2], blocker=19), obstacle, clearance=12, **band)
    out["seam blocker at h_hi + clearance + 1"] = case(seam([1, 2], blocker=20), level7(12), clearance=12, **band)

    # a band astride h = 0: the floor at z = -2, free up to z = 7
    g = np.full((16, 8, 8), FREE, np.uint32)              # z = -8 .. 7
    g[:6] = UNKNOWN
    g[6] = FLOOR

    def astride(m):
        assert all(fields(c) == (2, 2, 8, 1, 8, 2) for c in m.cells[0]), m.cells[0][0]   # window -4 .. 6: eight free cells above
        q = m.query([(1, 1, 3), (1, 1, -4)], 1.0)
        assert q["above"].tolist() == [5, -2] and q["surface"].tolist() == [-1.0, -1.0]

    out["band astride 0"] = case(from_grid(g, (0, 0, -1)), astride, h_lo=-4, h_hi=3, clearance=3, radius=4)

    # supports at h_lo, at h_hi and at h_hi + 1; a wall at h_hi + 1 over a support at h_hi
    g = np.full((16, 8, 8), FREE, np.uint32)
    g[2, 0, 0] = g[5, 0, 1] = g[6, 0, 2] = g[5, 0, 3] = FLOOR
    g[6, 0, 3] = KERB

    def edges(m):
        got = [fields(m.cells[0, cu]) for cu in range(5)]
        assert got == [(0, 0, 8, 1, 4, 0), (3, 3, 8, 1, 1, 0), (NO, NO, 0, 0, 0, 0), (NO, 3, 0, 2 | 8, 0, 0), (NO, NO, 0, 0, 0, 0)], got

    out["band edges"] = case(from_grid(g), edges, h_lo=2, h_hi=5, clearance=1, max_step=10, radius=2)
    return out


# 3 ---- cell rules
def rules():
    g = np.full((8, 8, 8), FREE, np.uint32)
    g[0] = FLOOR
    g[1, 1, 1] = MOVING
    g[0, 2, 2] = KERB
    g[0, 3, 3] = HIGH
    out = {}
    base = dict(h_lo=0, h_hi=7, clearance=2, radius=1)

    def expect(moving, kerb, high):
        def check(m):
            got = [fields(m.cells[0, k * 9]) for k in range(4)]
            assert got == [(0, 0, 8, 1, 7, 0), moving, kerb, high], got
        return check

    plain, blocked = (0, 0, 8, 1, 7, 0), (NO, 0, 0, 2 | 8, 0, 0)
    out["rules plain"] = case(bricks_of({(0, 0, 0): g}), expect((NO, 1, 0, 2 | 8, 0, 0), blocked, blocked), **base)
    out["rules ignore movable"] = case(bricks_of({(0, 0, 0): g}), expect(plain, blocked, blocked), ignore_movable=True, **base)
    out["rules label 40"] = case(bricks_of({(0, 0, 0): g}), expect((NO, 1, 0, 2 | 8, 0, 0), blocked, (0, 0, 40, 1, 7, 0)),
                                 **dict(base, support_labels=[8, 40]))
    # a span of 4095 cells over three archived bricks: the floor at z = 0, free bricks at bz = 100 and 511
    floor = np.full((8, 8, 8), FREE, np.uint32)
    floor[0] = FLOOR
    tall = bricks_of({(0, 0, 0): floor, (0, 0, 100): np.full((8, 8, 8), FREE, np.uint32), (0, 0, 511): np.full((8, 8, 8), FREE, np.uint32)})

    def saturated(headroom):
        def check(m):
            assert all(fields(c) == (0, 0, 8, 1, headroom, 255) for c in m.cells[0]), m.cells[0][0]
        return check

    out["saturation"] = case(tall, saturated(7), h_lo=0, h_hi=4095, clearance=5, radius=1)
    out["saturation unknown passable"] = case(tall, saturated(255), h_lo=0, h_hi=4095, clearance=255, radius=1, unknown_passable=True)
    return out


# 4 ---- steps across the tiles' sides: floors at z = 1, 4 and 5 in three of four tiles
def steps():
    def floor(z):
        g = np.full((8, 8, 8), FREE, np.uint32)
        g[:z] = UNKNOWN
        g[z] = FLOOR
        return g

    arch = bricks_of({(0, 0, 0): floor(1), (1, 0, 0): floor(4), (0, 1, 0): floor(5)})

    def expect(n_step, marked):
        def check(m):
            assert m.coords.tolist() == [[0, 0], [1, 0], [0, 1]] and m.info["n_step"] == m.info["n_lethal"] == n_step
            for i, j, want in marked:
                assert (column(m, i, j)[0]["cls"] >> 2) & 1 == want, (i, j)
        return check

    # only the higher side; the tile (1, 1) is absent: no relation at (15, 7) or (7, 15); 3 <= max_step 3: no step at all
    seen = [(8, 3, 1), (7, 3, 0), (3, 8, 1), (3, 7, 0), (15, 7, 0), (7, 15, 0), (9, 3, 0)]
    band = dict(h_lo=0, h_hi=7, clearance=1, radius=8)
    return {"steps max_step 2": case(arch, expect(16, seen), max_step=2, **band),
            "steps max_step 0": case(arch, expect(16, seen), max_step=0, **band),
            "steps max_step 3": case(arch, expect(8, [(8, 3, 0), (3, 8, 1)]), max_step=3, **band)}


# 5 ---- distances
def flat(tiles, pillars=(), holes=()):
    """a floor at z = 0 with free cells above in the tiles given; pillars: columns with a wall at z = 1; holes: columns of
    unknown cells"""
    words = {}
    for bu, bv in tiles:
        g = np.full((8, 8, 8), FREE, np.uint32)
        g[0] = FLOOR
        words[(bu, bv, 0)] = g
    for i, j in pillars:
        words[(i >> 3, j >> 3, 0)][1, j & 7, i & 7] = KERB
    for i, j in holes:
        words[(i >> 3, j >> 3, 0)][:, j & 7, i & 7] = UNKNOWN
    return bricks_of(words)


def distances():
    out = {}
    band = dict(h_lo=0, h_hi=3, clearance=1)

    def d2_are(pairs):
        def check(m):
            got = [column(m, i, j)[1] for i, j, _ in pairs]
            assert got == [w for _, _, w in pairs], got
        return check

    row = flat([(k, 0) for k in range(5)], pillars=[(20, 3)])
    out["row of five R 8"] = case(row, d2_are([(20, 3, 0), (28, 3, 64), (28, 4, NONE), (12, 3, 64), (12, 2, NONE), (25, 7, 41)]), radius=8, **band)
    out["row of five R 16"] = case(row, d2_are([(36, 3, 256), (36, 4, NONE), (4, 3, 256), (4, 2, NONE), (3, 3, NONE), (30, 0, 109)]), radius=16,
                                   **band)
    out["x wrap"] = case(flat([(0, 0)], pillars=[(7, 2)]), d2_are([(0, 3, 50), (0, 2, 49), (6, 3, 2)]), radius=8, **band)
    gap = flat([(0, 0), (1, 0), (3, 0), (4, 0)], pillars=[(15, 3)])
    out["tile missing between"] = case(gap, d2_are([(24, 3, 81), (31, 3, 256), (32, 3, NONE), (0, 3, 225)]), radius=16, **band)
    out["absent is lethal"] = case(gap, d2_are([(24, 3, 1), (31, 3, 16), (27, 3, 16), (15, 3, 0), (14, 3, 1), (35, 4, 16), (35, 3, 16)]), radius=16,
                                   absent_is_lethal=True, **band)
    out["none is lethal"] = case(flat([(0, 0), (1, 0)], holes=[(9, 4)]), d2_are([(9, 4, 0), (3, 4, 36), (9, 0, 16), (0, 4, NONE)]), radius=8,
                                 none_is_lethal=True, **band)
    plate = flat(list(itertools.product(range(5), range(5))), pillars=[(20, 20)])
    out["diagonal"] = case(plate, d2_are([(31, 31, 242), (32, 32, NONE), (9, 9, 242), (8, 8, NONE), (31, 9, 242), (20, 36, 256), (21, 36, NONE)]),
                           radius=16, **band)
    return out


# 6 ---- which tiles exist
def existence():
    free = np.full((8, 8, 8), FREE, np.uint32)
    arch = bricks_of({(0, 0, 0): free, (1, 0, 5): free, (2, 0, 1): free, (0, 3, 0): free, (-2, -1, 0): free})

    def tiles_are(want):
        def check(m):
            assert m.coords.tolist() == want and m.info["n_tiles"] == len(want) and m.info["n_none"] == 64 * len(want)
        return check

    band = dict(h_lo=0, h_hi=5, clearance=3, radius=4)       # the window ends at z = 8, the first cell of bz = 1
    return {"existence": case(arch, tiles_are([[-2, -1], [0, 0], [2, 0], [0, 3]]), **band),
            "existence shorter window": case(arch, tiles_are([[-2, -1], [0, 0], [0, 3]]), **dict(band, clearance=2)),
            "existence box": case(arch, tiles_are([[0, 0], [2, 0]]), box=((0, -1), (2, 2)), **band),
            "existence empty box": case(arch, tiles_are([]), box=((0, 0), (-1, 5)), **band)}


# 7 ---- the int16 edge: int16_edge()'s bricks, those a key overflow would make somebody's neighbour free - class 0, lethal
# under none_is_lethal - and the others solid floor through and through: ground in every orientation at clearance 0
def edge():
    e = int16_edge()
    lonely = set(e["lonely"])
    hdr, cells = e["hdr"], e["cells"].copy()
    coord = [(int(h["bx"]), int(h["by"]), int(h["bz"])) for h in hdr]
    for k, b in enumerate(coord):
        if b not in lonely:
            cells[k] = FLOOR

    def expect(up, fenced):
        au, av = (1 if up[0] == 0 else 0), (1 if up[0] == 2 else 2)

        def check(m):
            free = {(b[au], b[av]) for b in lonely}
            assert len(m.coords) >= 8
            for r, t in enumerate(m.coords.tolist()):
                if tuple(t) in free:
                    assert (m.d2[r] == 0).all() and (m.cells["cls"][r] == 8).all(), t
                elif fenced:       # no column of a tile is more than four columns from its side
                    assert (m.d2[r] >= 1).all() and (m.d2[r] <= 16).all() and (m.cells["cls"][r] == 1).all(), t
                else:              # nothing near: a key that overflowed would bring a lethal neighbour
                    assert (m.d2[r] == NONE).all() and (m.cells["cls"][r] == 1).all(), t
        return check

    out = {"int16 edge z": case((hdr, cells), expect((2, 1), False), h_lo=0, h_hi=135, clearance=0, radius=16, none_is_lethal=True),
           "int16 edge x": case((hdr, cells), expect((0, -1), False), up=(0, -1), h_lo=-200, h_hi=-1, clearance=0, radius=16, none_is_lethal=True),
           "int16 edge absent": case((hdr, cells), expect((1, 1), True), up=(1, 1), h_lo=0, h_hi=300, clearance=0, radius=9, none_is_lethal=True,
                                     absent_is_lethal=True)}
    g = np.full((8, 8, 8), UNKNOWN, np.uint32)
    g[6], g[7] = FLOOR, FREE
    top = bricks_of({(0, 0, 32767): g})
    band = dict(h_lo=262136, h_hi=262143 + 50, clearance=5, radius=2)

    def beyond(want):
        def check(m):
            assert all(fields(c) == want for c in m.cells[0]), m.cells[0][0]
        return check

    # z = 262142 is relative 6; one free cell, then nothing but cells beyond the brick range: unknown.  The band holds 6 + 50
    # unknown cells, the window ends at relative 62.
    out["window beyond the range"] = case(top, beyond((6, 6, 8, 1, 56, 56)), unknown_passable=True, **band)
    out["window beyond the range, unknown blocks"] = case(top, beyond((NO, 6, 0, 2 | 8, 0, 56)), **band)
    return out


# 8 ---- the random archive: every flag combination, two radii, three orientations
ORIENTATIONS = {(2, 1): dict(h_lo=2, h_hi=12), (1, -1): dict(h_lo=-20, h_hi=3), (0, 1): dict(h_lo=-5, h_hi=20)}


def random_variants():
    out = []
    for up, (up_, ip, nl, al), radius in itertools.product(ORIENTATIONS, [(u, i, n, a) for u in (False, True) for i in (False, True)
                                                                          for n in (False, True) for a in (False, True)], (3, 16)):
        out.append(dict(up=up, clearance=2, max_step=1, radius=radius, support_labels=SUPPORT, unknown_passable=up_, ignore_movable=ip,
                        none_is_lethal=nl, absent_is_lethal=al, **ORIENTATIONS[up]))
    out.append(dict(up=(2, 1), h_lo=0, h_hi=15, clearance=1, max_step=0, radius=9, support_labels=[7, 8], box=((0, -1), (1, 1))))
    return out


# 9 ---- footprints: four tiles meet at column (0, 0); the tile (0, 0) is higher, a pillar stands at (-2, 1)
def corner():
    g = np.full((8, 16, 16), FREE, np.uint32)             # columns -8 .. 7
    g[0] = FLOOR
    g[1:3, 8:, 8:] = UNKNOWN
    g[3, 8:, 8:] = FLOOR
    g[0:3, 8:, 8:] = UNKNOWN
    g[1, 9, 6] = KERB
    return from_grid(g, (-1, -1, 0))


def corner_case(skip=()):
    hdr, cells = corner()
    if skip:
        keep = np.array([(int(h["bx"]), int(h["by"])) not in skip for h in hdr])
        hdr, cells = hdr[keep], cells[keep]
    return case((hdr, cells), None, h_lo=0, h_hi=6, clearance=2, max_step=1, radius=8)


def footprint_set():
    """FOOTPRINT records (center_u, center_v, dir_u, dir_v, half_len, half_wid): axis-aligned and rotated over the corner, one
    that hangs over the side of the archive, one too large, non-finite ones, one with no heading, one far away"""
    inf, nan = np.inf, np.nan
    return np.array([(0.0, 0.0, 1.0, 0.0, 2.6, 1.2), (0.3, -0.2, 0.6, 0.8, 3.4, 1.7), (-1.0, 1.0, -0.8, 0.6, 2.0, 2.0), (7.0, 0.0, 1.0, 0.0, 3.0, 1.0),
                     (0.0, 0.0, 0.0, 1.0, 40.0, 24.5), (0.0, 0.0, 0.0, 1.0, 40.0, 24.0), (nan, 0.0, 1.0, 0.0, 1.0, 1.0), (0.0, 0.0, 1.0, 0.0, inf, 1.0),
                     (0.0, 0.0, 0.1, 0.1, 1.0, 1.0), (5000.5, -3.0, 1.0, 0.0, 2.0, 2.0), (3.0e8, 0.0, 1.0, 0.0, 2.0, 2.0), (2.5, 2.5, 1.0, 0.0, 0.0, 0.0),
                     (0.0, 0.0, 1.0, 0.0, 0.4, 0.4)], np.float32).view(FOOTPRINT).reshape(-1)


# 10 ---- the block whose ground layer the world's must agree with: 32 cells an axis, the ring at rest
def block_config():
    from semantic_dsp_map_amd import synth
    cfg = dict(synth.CONFIGS["T0"])
    cfg.update(x_n=5, y_n=5, z_n=5, p_n=1, voxel_size=0.25)
    return cfg


BLOCK_BAND = dict(h_lo=2, h_hi=12, clearance=3, max_step=1)      # block heights; h_hi + clearance < 32
BLOCK_RADIUS = 8


def block_scene(up):
    """-> (occ int8, label uint8, track uint16) [z, y, x], 32 cells an axis: a road at height 4, a platform at height 7 over
    one quadrant (a kerb of three cells), boxes on the road, a parked car, a patch nobody has seen, a roof too low to pass
    under; `up`: (axis, sign), the heights counted as the ground layer counts them"""
    from semantic_dsp_map_amd import synth
    N = 32
    occ, label, track = np.zeros((N, N, N), np.int8), np.zeros((N, N, N), np.uint8), np.zeros((N, N, N), np.uint16)   # [h, v, u]

    def put(sl, o, l=0, t=0):
        occ[sl], label[sl], track[sl] = o, l, t

    road, box = (1, synth.LABEL_ROAD, synth.TRACK_ROAD), (1, synth.LABEL_BUILDING, synth.TRACK_BUILDING)
    put((slice(0, 4),), -1)
    put((4,), *road)
    put((slice(0, 7), slice(16, 32), slice(16, 32)), -1)
    put((7, slice(16, 32), slice(16, 32)), *road)
    put((slice(5, 9), slice(3, 6), slice(20, 27)), *box)
    put((slice(5, 7), slice(22, 24), slice(2, 4)), *box)
    put((5, slice(10, 12), slice(10, 13)), 1, synth.LABEL_CAR, 3)
    put((slice(None), slice(20, 23), slice(6, 9)), -1)
    put((6, slice(12, 16), slice(0, 16)), *box)
    put((slice(8, 10), slice(26, 29), slice(26, 29)), -1)
    axis, sign = up
    au, av = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    at = {axis: 0, av: 1, au: 2}
    perm = [at[2], at[1], at[0]]
    out = [np.ascontiguousarray(np.flip(a.transpose(perm), axis=2 - axis) if sign < 0 else a.transpose(perm)) for a in (occ, label, track)]
    return tuple(out)


def crafted():
    """name -> case, every crafted case (the random archive's variants and the footprints apart)"""
    out = {}
    for axis, sign, at in itertools.product((0, 1, 2), (1, -1), (-1, 0)):
        out["orientation %d %+d at %d" % (axis, sign, at)] = orientation(axis, sign, at)
    for part in (seams(), rules(), steps(), distances(), existence(), edge()):
        out.update(part)
    return out

