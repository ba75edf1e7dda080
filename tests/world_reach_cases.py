"""The crafted archives of the world reach tests: hand-written bricks (WORLD_BRICK headers in brick order and 512 words
each) with their starts, shared by tests/test_world_reach_ref.py (the two restatements against each other, no GPU) and
tests/test_world_reach_gpu.py (the library against them).  A case is a dict: hdr, cells, starts (world cells) and kw, the
build's keywords; some carry what the test asserts beyond equality."""
import itertools

import numpy as np

from tests import shape_cases as sc
from tests import world_io_ref as io

CFG = sc.config("A")              # the archive needs a map only as a handle: 4 cells an axis
MM = CFG["max_movable_track"]
FREE, UNKNOWN = 0, 0xFF000000
WALL = 1 << 24 | 8 << 16 | 65535  # occupied, a static track
MOVING = 1 << 24 | 7 << 16 | 3    # occupied, a movable track
assert 3 <= MM < 65535


def bricks_of(words):
    """`words` maps a brick coordinate (bx, by, bz) to its uint32 [8, 8, 8] words indexed [cz, cy, cx] -> (hdr, cells) in
    brick order"""
    coord = sorted(words, key=lambda b: (b[2], b[1], b[0]))
    hdr = io.make_headers(np.array(coord, np.int64).reshape(-1, 3))
    cells = np.stack([np.asarray(words[b], np.uint32).reshape(512) for b in coord]) if coord else np.zeros((0, 512), np.uint32)
    return hdr, cells


def from_grid(grid, lo_brick=(0, 0, 0), skip=()):
    """a dense word grid [z, y, x] whose extents are multiples of 8, its cell (0, 0, 0) the first cell of brick lo_brick,
    without the bricks (absolute coordinates) in `skip`"""
    Z, Y, X = grid.shape
    words = {}
    for bz, by, bx in itertools.product(range(Z // 8), range(Y // 8), range(X // 8)):
        b = (lo_brick[0] + bx, lo_brick[1] + by, lo_brick[2] + bz)
        if b not in skip:
            words[b] = grid[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]
    return bricks_of(words)


def case(hdr_cells, starts, **kw):
    return dict(hdr=hdr_cells[0], cells=hdr_cells[1], starts=np.asarray(starts, np.int64).reshape(-1, 3), kw=kw)


# 1 ---- one free brick, the start in a corner
def one_brick(at):
    at = np.asarray(at, np.int64)
    return case(bricks_of({tuple(at.tolist()): np.full((8, 8, 8), FREE, np.uint32)}), [at * 8])


def closed_form(d, face):
    """the cost of offset d = (dx, dy, dz) >= 0 in free space"""
    lo, mid, hi = sorted(int(v) for v in d)
    return 10 * (lo + mid + hi) if face else 17 * lo + 14 * (mid - lo) + 10 * (hi - mid)


# 2 ---- 2 x 2 x 2 bricks astride 0: the cell planes x = -1, y = -1, z = -1 are walls, one hole
def rooms(kind):
    g = np.full((16, 16, 16), FREE, np.uint32)   # cell c at index c + 8
    g[7, :, :] = g[:, 7, :] = g[:, :, 7] = WALL
    if kind == "face":       # through the wall x = -1, in the middle of a face between two bricks
        g[8 + 3, 8 + 3, 7] = FREE
    elif kind == "edge":     # round the line x = y = -1 where four bricks meet
        g[8 + 4, 7:9, 7:9] = FREE
    elif kind == "corner":   # round the point where the eight bricks meet
        g[7:9, 7:9, 7:9] = FREE
    c = case(from_grid(g, (-1, -1, -1)), [(5, 6, 4)])
    # the walls are one cell thick on the negative side: a hole opens into the rooms it touches with a face, so into those
    # with at most one negative axis; the cells of the hole itself are reached across the edge (14) or the corner (17)
    c["rooms_reached"] = {"face": 2, "edge": 3, "corner": 4}[kind]
    return c


# 3 ---- 3 x 3 x 3 bricks without the middle one
def shell(through_unknown, seed=5):
    rng = np.random.default_rng(seed)
    g = np.where(rng.random((24, 24, 24)) < 0.1, UNKNOWN, FREE).astype(np.uint32)
    g[4, 4, 0] = FREE
    return case(from_grid(g, (-1, -1, -1), skip=[(0, 0, 0)]), [(-8, -4, -4)], through_unknown=through_unknown)


# 4 ---- the late corner of tests/test_reach_gpu.py: its four tiles are the bricks (0, 1..2, 6..7)
def late_corner():
    from tests.test_reach_gpu import late_corner as block_case
    occ, starts, marks = block_case()       # occ [64, 32, 4]; cell words x | y << 2 | z << 7
    g = np.full((64, 32, 8), WALL, np.uint32)
    g[:, :, :4] = np.where(occ == 0, FREE, WALL)
    cell = lambda w: (w & 3, (w >> 2) & 31, w >> 7)  # noqa: E731
    c = case(from_grid(g), [cell(w) for w in starts])
    c["marks"] = [cell(w) for w in marks]   # c, f1, f2, d: 550, 560, 560, 564
    return c


# 5 ---- a corridor through 12 bricks in a row; a serpentine inside 2 x 2 bricks
def corridor():
    g = np.full((8, 8, 96), WALL, np.uint32)
    g[3, 3, :] = FREE
    return case(from_grid(g, (-5, 2, -1)), [(-40, 19, -5)])


def serpentine():
    g = np.full((8, 16, 16), WALL, np.uint32)
    g[2, 0::2, :] = FREE
    for k, y in enumerate(range(1, 16, 2)):
        g[2, y, 15 if k % 2 == 0 else 0] = FREE
    return case(from_grid(g, (-1, -1, 0)), [(-8, -8, 2)], face_connected=True)


# 6 ---- random: 4 x 4 x 2 bricks, three missing
RANDOM_SKIP = [(0, 1, 0), (2, 2, 1), (-1, 0, 1)]


def random_world(seed=11):
    rng = np.random.default_rng(seed)
    u = rng.random((16, 32, 32))
    g = np.full(u.shape, FREE, np.uint32)
    g[u < 0.4] = UNKNOWN
    g[u < 0.3] = WALL
    g[u < 0.1] = MOVING
    g[8, 12, 12] = g[3, 20, 5] = FREE
    return from_grid(g, (-1, -1, 0), skip=RANDOM_SKIP)


RANDOM_STARTS = [(4, 4, 8), (-3, 12, 3), (4, 4, 8)]


def random_variants():
    """the builds of the random archive: every combination of the three flags and inflate 0 / 1 / 2, a budget that cuts
    the field, a box that cuts the bricks"""
    out = []
    for face, tu, im, inflate in itertools.product((False, True), (False, True), (False, True), (0, 1, 2)):
        out.append(dict(through_unknown=tu, ignore_movable=im, inflate=inflate, face_connected=face))
    out.append(dict(through_unknown=True, ignore_movable=True, max_cost=120))
    out.append(dict(through_unknown=True, ignore_movable=True, max_cost=95, face_connected=True))
    out.append(dict(through_unknown=True, ignore_movable=True, box=((0, -1, 0), (2, 1, 1))))
    out.append(dict(through_unknown=True, inflate=1, box=((-1, -1, 1), (1, 2, 1))))
    return out


def pillars(inflate, face, seed=3):
    """3 x 3 x 2 bricks, one missing, 0.4 % obstacles (half of them movable) and some unknown cells: what an inflation
    leaves is still a connected field (the random archive's inflated fields are all but empty)"""
    rng = np.random.default_rng(seed)
    u = rng.random((16, 24, 24))
    g = np.full(u.shape, FREE, np.uint32)
    g[u < 0.05] = UNKNOWN
    g[u < 0.004] = WALL
    g[u < 0.002] = MOVING
    g[2:7, 2:7, 2:7] = g[11:16, 18:23, 18:23] = FREE   # round the two starts
    return case(from_grid(g, (-2, -1, -1), skip=[(-1, 0, 0)]), [(-12, -4, -4), (4, 12, 5)], inflate=inflate, face_connected=face,
                through_unknown=True)


def ball(inflate, skip):
    """one obstacle cell in the corner of a brick where eight bricks meet (seven, with skip)"""
    g = np.full((16, 16, 16), FREE, np.uint32)
    g[8, 8, 8] = WALL
    return case(from_grid(g, (-1, -1, -1), skip=[(-1, -1, -1)] if skip else []), [(5, 5, 5)], inflate=inflate)


# 7 ---- more bricks than a scan tile of 2048: a plate of 46 x 46 bricks, only the cell layer cz = 3 free
def plate(face):
    n = 46
    g = np.full((8, 8 * n, 8 * n), WALL, np.uint32)
    g[3] = FREE
    return case(from_grid(g, (-20, -23, 4)), [(17, 3, 35)], face_connected=face)


# 8 ---- the int16 edge: per axis and end a free brick at the edge, and the brick a key overflow would make its neighbour
def int16_edge():
    words, starts, lonely = {}, [], []
    free = np.full((8, 8, 8), FREE, np.uint32)
    for a in range(3):
        for k, (edge, other) in enumerate(((32767, -32768), (-32768, 32767))):
            b, q = [10 * a + 4 * k, 10 * a + 4 * k + 1, 10 * a + 4 * k + 2], None
            b[a] = edge
            nxt = (a + 1) % 3              # the axis whose key field a carry (or borrow) out of axis a's reaches
            q = list(b)
            q[a], q[nxt] = other, b[nxt] + (1 if edge > 0 else -1)
            words[tuple(b)], words[tuple(q)] = free, free
            starts.append([8 * v + 3 for v in b])
            lonely.append(tuple(q))
    c = case(bricks_of(words), starts)
    c["lonely"] = lonely
    return c


def crafted():
    """name -> case, every crafted case at full size (the random archive's variants apart)"""
    out = {"one brick": one_brick((0, 0, 0)), "one brick at -1": one_brick((-1, -1, -1)), "late corner": late_corner(),
           "corridor": corridor(), "serpentine": serpentine(), "int16 edge": int16_edge()}
    for kind in ("face", "edge", "corner"):
        out["rooms " + kind] = rooms(kind)
    for tu in (False, True):
        out["shell through_unknown=%s" % tu] = shell(tu)
    for face in (True, False):
        out["plate face=%s" % face] = plate(face)
    for inflate, face in ((1, False), (2, False), (2, True)):
        out["pillars inflate=%d face=%s" % (inflate, face)] = pillars(inflate, face)
    for inflate, skip in ((1, False), (1, True), (2, False), (2, True)):
        out["ball inflate=%d skip=%s" % (inflate, skip)] = ball(inflate, skip)
    return out


def sample_goals(ref, n, seed):
    """world cells: reached, unreached and blocked cells of the field, its starts' neighbourhood, and cells of no brick"""
    rng = np.random.default_rng(seed)
    base = ref.coords.astype(np.int64) * 8
    picks = []
    for mask in (ref.cost != 0xFFFFFFFF, ref.trav & (ref.cost == 0xFFFFFFFF), ~ref.trav):
        at = np.argwhere(mask)
        if len(at):
            at = at[rng.choice(len(at), min(n, len(at)), replace=False)]
            w = at[:, 1]
            picks.append(base[at[:, 0]] + np.stack([w & 7, (w >> 3) & 7, w >> 6], 1))
    far = np.array([[int(base[:, 0].max()) + 16, int(base[0, 1]), int(base[0, 2])], [0, 0, int(base[:, 2].min()) - 9]], np.int64)
    return np.concatenate(picks + [far])
