"""The crafted archives of the world ground reach tests: terrains written as a grid of floor heights, turned into bricks
with the helpers of tests/world_reach_cases.py, shared by tests/test_world_ground_reach_ref.py (the two restatements against
each other and against the values worked out by hand here, no GPU) and tests/test_world_ground_reach_gpu.py (the library
against them).  A case is a dict: hdr, cells, gkw - the ground build's keywords -, starts (world cells), kw - the reach
build's keywords - and `expect`, a function of a model that asserts the hand values.  Columns are (i_u, j_v)."""
import itertools

import numpy as np

from tests.world_ground_cases import FLOOR, SUPPORT
from tests.world_reach_cases import CFG, FREE, MM, UNKNOWN, from_grid, int16_edge, random_world

SIZE = np.float32(CFG["voxel_size"])
NO = 0xFFFFFFFF
WALL, HOLE = -2, -1                      # in a terrain: a solid column (an obstacle, lethal) / a column nobody has seen (class 0)
GROUND = dict(h_lo=0, h_hi=6, clearance=1, max_step=7, radius=4, support_labels=SUPPORT)
FILL = -0x80000000
assert MM >= 3


def axes(up):
    a = up[0]
    return a, (1 if a == 0 else 0), (1 if a == 2 else 2)


def cell(up, iu, iv, ga=77):
    """a world cell over column (iu, iv); ga: its coordinate along the up axis, which no answer depends on"""
    a, au, av = axes(up)
    g = [0, 0, 0]
    g[a], g[au], g[av] = ga, iu, iv
    return g


def terrain(H, lo_tile=(0, 0), up=(2, 1), skip=()):
    """H [v, u]: the floor's height 0 .. 6 per column (solid from height 0 up to it, free above), WALL or HOLE; the grid's
    column (0, 0) is the first column of tile lo_tile; `skip`: tiles (bu, bv) left out -> (hdr, cells)"""
    H = np.asarray(H, np.int64)
    nv, nu = H.shape
    W = np.full((8, nv, nu), FREE, np.uint32)                            # [height, v, u]
    for h in range(8):
        W[h][H >= h] = FLOOR
    W[:, H == WALL] = FLOOR
    W[:, H == HOLE] = UNKNOWN
    a, au, av = axes(up)
    pos = {a: 0, av: 1, au: 2}
    grid = W.transpose(pos[2], pos[1], pos[0])                          # [z, y, x]
    lo = [0, 0, 0]
    lo[au], lo[av] = lo_tile
    if up[1] < 0:                                                       # height h is coordinate -1 - h: the brick below 0
        grid = np.flip(grid, axis=2 - a)
        lo[a] = -1

    def brick(t):
        b = [0, 0, 0]
        b[a], b[au], b[av] = lo[a], t[0], t[1]
        return tuple(b)

    return from_grid(np.ascontiguousarray(grid), tuple(lo), skip=[brick(t) for t in skip])


def case(hdr_cells, starts, expect=None, up=(2, 1), gkw=None, **kw):
    g = dict(GROUND, up=up)
    g.update(gkw or {})
    return dict(hdr=hdr_cells[0], cells=hdr_cells[1], gkw=g, up=up, starts=np.asarray(starts, np.int64).reshape(-1, 3), kw=kw, expect=expect)


def cost_at(m, iu, iv):
    return int(m.cost[m.where(iu, iv)])


def ask(m, up, cols):
    return m.query([cell(up, iu, iv) for iu, iv in cols], SIZE)


def path_of(m, up, iu, iv, max_len=400):
    rows, lens = m.paths([cell(up, iu, iv)], max_len, FILL)
    return rows[0, :lens[0]].tolist(), int(lens[0])


def path_sum(m, up, cells):
    """the cost of a path, goal first: the moves' weights and the penalty of every column entered on the way from the start"""
    a, au, av = axes(up)
    total = 0
    for p, q in zip(cells[:-1], cells[1:]):                             # q -> p is a move of the way from the start
        du, dv = abs(p[au] - q[au]), abs(p[av] - q[av])
        assert max(du, dv) == 1
        total += (14 if du and dv else 10) + int(m.pen[m.where(p[au], p[av])])
    return total


# 1 ---- one flat tile, the start in a corner
def one_tile(face, at=(0, 0)):
    u0, v0 = 8 * at[0], 8 * at[1]

    def expect(m):
        want = np.array([[10 * (cu + cv) if face else 10 * max(cu, cv) + 4 * min(cu, cv) for cu in range(8)] for cv in range(8)])
        assert m.coords.tolist() == [list(at)] and np.array_equal(m.cost.reshape(8, 8), want)
        assert m.info["n_starts_used"] == 1 and m.info["n_traversable"] == m.info["n_reached"] == 64 and m.info["max_cost_reached"] == want.max()
        q = ask(m, (2, 1), [(u0 + 7, v0 + 7), (u0, v0), (u0 + 3, v0)])
        assert q["next"].tolist() == [1 if face else 0, 4, 3] and q["status"].tolist() == [0, 0, 0] and q["level"].tolist() == [0, 0, 0]
        assert q["metres"][0] == np.float32(want.max()) * (SIZE * np.float32(0.1)) and q["col"].tolist()[0] == [u0 + 7, v0 + 7]
        cells, n = path_of(m, (2, 1), u0 + 7, v0 + 7)
        if face:   # the smallest move number first: down along v, then along u
            assert cells == [[u0 + 7, v0 + k, 1] for k in range(7, 0, -1)] + [[u0 + k, v0, 1] for k in range(7, -1, -1)]
        else:
            assert cells == [[u0 + k, v0 + k, 1] for k in range(7, -1, -1)]
        assert n == len(cells) and path_sum(m, (2, 1), cells) == want.max()

    return case(terrain(np.zeros((8, 8)), at), [cell((2, 1), u0, v0)], expect, face_connected=face)


# 2 ---- seams
def seams():
    out = {}

    def two(m):
        assert len(m.coords) == 2 and m.info["n_reached"] == 128
    flat = np.zeros((8, 16))

    def in_u(m):
        two(m)
        assert cost_at(m, 15, 3) == 10 * 15 + 4 * 3 and cost_at(m, 8, 0) == 80 and ask(m, (2, 1), [(8, 1)])["next"][0] == 0

    def in_v(m):
        two(m)
        assert cost_at(m, 3, 15) == 10 * 15 + 4 * 3 and cost_at(m, 0, 8) == 80
    out["seam in u"] = case(terrain(flat), [cell((2, 1), 0, 0)], in_u)
    out["seam in v"] = case(terrain(flat.T), [cell((2, 1), 0, 0)], in_v)

    def corner(up):
        def expect(m):
            assert len(m.coords) == 4 and cost_at(m, 8, 8) == 14 and cost_at(m, 8, 7) == 10 and cost_at(m, 15, 15) == 8 * 14
            assert ask(m, up, [(8, 8)])["next"][0] == 0 and m.info["n_reached"] == 256
            cells, n = path_of(m, up, 9, 9)
            h = 1 if up[1] > 0 else -2                                  # the base stands at height 1
            assert cells == [cell(up, 9, 9, h), cell(up, 8, 8, h), cell(up, 7, 7, h)]
        return expect
    out["four tiles round a corner"] = case(terrain(np.zeros((16, 16))), [cell((2, 1), 7, 7)], corner((2, 1)))
    for a in range(3):
        up = (a, -1)
        out["four tiles round a corner, up %d -1" % a] = case(terrain(np.zeros((16, 16)), up=up), [cell(up, 7, 7)], corner(up), up=up)

    def diagonal_only(m):
        assert m.coords.tolist() == [[0, 0], [1, 1]] and m.info["n_reached"] == 64 and m.info["n_traversable"] == 128
        q = ask(m, (2, 1), [(8, 8), (8, 7)])
        assert q["status"].tolist() == [1, 3] and q["cost"].tolist() == [NO, NO] and q["next"].tolist() == [255, 255]
    out["two diagonal tiles"] = case(terrain(np.zeros((16, 16)), skip=[(1, 0), (0, 1)]), [cell((2, 1), 7, 7)], diagonal_only)
    return out


# 3 ---- the late corner: tile (1, 1) must be woken across the corner of tile (0, 0)
LATE_MARKS = dict(c=(7, 7), f1=(8, 7), f2=(7, 8), d=(8, 8))


def late_corner():
    """2 x 2 tiles of walls with corridors.  Start A's wave crosses from tile (0, 0) into tile (1, 0) and back before it
    runs up the column u = 7 to c = (7, 7), the corner column of tile (0, 0): it arrives there in the third round, at cost
    130.  The side neighbours f1 = (8, 7) and f2 = (7, 8) of c have had cost 140 since the first round, each from a start of
    its own at the end of a corridor of 14 moves inside its own tile; from them d = (8, 8), the only column of tile (1, 1),
    stood at 150 after the second round.  c's arrival lowers neither f1 nor f2, so neither of their tiles wakes tile (1, 1)
    again: d falls to 144, by the diagonal from c, only if tile (0, 0) wakes the tile across its corner."""
    H = np.full((16, 16), WALL, np.int64)
    way_a = [(5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (9, 1), (9, 2), (8, 2)] + [(7, v) for v in range(2, 8)]
    way_1 = [(8 + k, 7) for k in range(8)] + [(15, 6)] + [(15 - k, 5) for k in range(6)]        # f1 .. its start (10, 5)
    way_2 = [(v, u) for u, v in way_1]                                                           # f2 .. its start (5, 10)
    for u, v in way_a + way_1 + way_2 + [LATE_MARKS["d"]]:
        H[v, u] = 0
    starts = [cell((2, 1), *way_a[0]), cell((2, 1), *way_1[-1]), cell((2, 1), *way_2[-1])]

    def expect(m):
        got = {k: cost_at(m, *q) for k, q in LATE_MARKS.items()}
        assert got == dict(c=130, f1=140, f2=140, d=144) and m.info["n_starts_used"] == 3
        assert ask(m, (2, 1), [LATE_MARKS["d"]])["next"][0] == 0

    return case(terrain(H), starts, expect)


def emulate_rounds(m, corners):
    """the rounds of the build on a SparseReach `m`, tile by tile: every active tile relaxes its own columns to rest from
    the costs at the round's start, then wakes the tiles whose halo holds a column it lowered - across sides, and across
    corners only if `corners` -> {column: cost}"""
    INF = 1 << 62
    cost = {c: INF for c in m.col}
    active = set()
    seeds = [c for c in m._start_columns(m.start_cells) if c in m.col]
    for c in seeds:
        cost[c] = 0
        for du, dv in itertools.product((-1, 0, 1), repeat=2):
            active.add(((c[0] >> 3) + du, (c[1] >> 3) + dv))
    rounds = 0
    while active:
        rounds += 1
        assert rounds < 1000
        old, woken = dict(cost), set()
        for t in sorted(active):
            own = [c for c in m.col if (c[0] >> 3, c[1] >> 3) == t]
            local = {c: old[c] for c in own}
            changed = True
            while changed:
                changed = False
                for c in own:
                    for k, du, dv in m.moves:
                        q = (c[0] + du, c[1] + dv)
                        if m.may(c, du, dv):
                            via = local.get(q, old.get(q, INF)) + (14 if du and dv else 10) + m.col[c][1]
                            if via < local[c]:
                                local[c], changed = via, True
            for c in own:
                if local[c] < old[c]:
                    cost[c] = local[c]
                    for du, dv in itertools.product((-1, 0, 1), repeat=2):
                        sees = (du != 0 or dv != 0) and (du == 0 or (c[0] & 7) == (0 if du < 0 else 7)) and (dv == 0 or (c[1] & 7) == (0 if dv < 0 else 7))
                        if sees and (corners or du == 0 or dv == 0):
                            woken.add((t[0] + du, t[1] + dv))
        active = {t for t in woken if tuple(t) in m.rank}
    return {c: (v if v < INF else None) for c, v in cost.items()}


# 4 ---- climb
def climbs():
    out = {}

    def row(heights):
        H = np.full((8, 8), WALL, np.int64)
        H[0, :len(heights)] = heights
        return terrain(H)
    start = [cell((2, 1), 0, 0)]
    ramp = list(range(7))

    def ramp_up(m):
        assert cost_at(m, 6, 0) == 60 and ask(m, (2, 1), [(6, 0)])["level"][0] == 6 and path_of(m, (2, 1), 2, 0)[0] == [[2, 0, 3], [1, 0, 2], [0, 0, 1]]

    def ramp_no(m):
        assert m.info["n_reached"] == 1 and ask(m, (2, 1), [(1, 0)])["status"][0] == 1
    out["ramp max_climb 1"] = case(row(ramp), start, ramp_up, max_climb=1)
    out["ramp max_climb 0"] = case(row(ramp), start, ramp_no, max_climb=0)

    def kerb_blocks(m):
        assert m.info["n_reached"] == 2 and ask(m, (2, 1), [(2, 0)])["status"][0] == 1

    def kerb_passes(m):
        assert cost_at(m, 3, 0) == 30
    out["kerb of 2 max_climb 1"] = case(row([0, 0, 2, 2]), start, kerb_blocks, max_climb=1)
    out["kerb of 2 max_climb 2"] = case(row([0, 0, 2, 2]), start, kerb_passes, max_climb=2)
    H = np.full((8, 8), WALL, np.int64)
    H[0:2, 0:2] = [[0, 2], [0, 0]]                                      # (1, 0) stands two cells higher

    def one_too_high(m):   # the diagonal (0, 0) -> (1, 1) would cost 14
        assert cost_at(m, 1, 1) == 20 and ask(m, (2, 1), [(1, 1)])["next"][0] == 3 and ask(m, (2, 1), [(1, 0)])["status"][0] == 1

    def all_low_enough(m):
        assert cost_at(m, 1, 1) == 14 and cost_at(m, 1, 0) == 10
    out["diagonal with one column too high"] = case(terrain(H), start, one_too_high, max_climb=1)
    out["diagonal with max_climb 2"] = case(terrain(H), start, all_low_enough, max_climb=2)

    def step_bit(m):   # the ground build marks (2, 0) as a step of three over max_step 1: lethal, whatever max_climb says
        q = ask(m, (2, 1), [(1, 0), (2, 0), (3, 0)])
        assert q["status"].tolist() == [0, 2, 1] and q["level"].tolist() == [0, 3, 3]
    out["lethal by the step bit"] = case(row([0, 0, 3, 3]), start, step_bit, gkw=dict(max_step=1), max_climb=6)
    return out


# 5 / 6 / 7 ---- clearance, penalty, budget: a strip of `rows` rows in a sea of unseen columns, one pillar at (4, 1)
def strip(rows):
    H = np.full((8, 8), HOLE, np.int64)
    H[:rows] = 0
    H[1, 4] = WALL
    return terrain(H)


def clearances():
    out = {}
    start, R3 = [cell((2, 1), 0, 1)], dict(radius=3)

    def open_(m):   # round the pillar: two straight moves, a diagonal, two straight, a diagonal, one straight
        assert cost_at(m, 7, 1) == 78 and ask(m, (2, 1), [(4, 1)])["status"][0] == 2

    def closed(m):   # the column u = 4 is within distance 1 of the pillar
        assert ask(m, (2, 1), [(7, 1), (4, 0), (3, 1)])["status"].tolist() == [1, 2, 2]
    for d in (0, 1):
        out["clearance min_d2 %d" % d] = case(strip(3), start, open_, gkw=R3, min_d2=d)
    for d in (2, 4, 9):
        out["clearance min_d2 %d" % d] = case(strip(3), start, closed, gkw=R3, min_d2=d)

    def only_far(m):   # R^2 + 1: the columns whose d2 reads NONE - u = 0 whole, (1, 0), (1, 2), (7, 0), (7, 2)
        assert m.info["n_traversable"] == 7 and m.info["n_reached"] == 5 and cost_at(m, 1, 0) == 20
        assert ask(m, (2, 1), [(1, 1), (7, 0)])["status"].tolist() == [2, 1]
    out["clearance min_d2 R^2 + 1"] = case(strip(3), start, only_far, gkw=R3, min_d2=10)
    return out


def penalties():
    out = {}
    start = [cell((2, 1), 0, 1)]

    def short(m):
        assert cost_at(m, 7, 1) == 78
        cells, n = path_of(m, (2, 1), 7, 1)
        assert n == 8 and path_sum(m, (2, 1), cells) == 78

    def long_(m):   # the way along row 0 or 2 enters three columns within sqrt(2) of the pillar: 78 + 15; row 3 is clear
        assert cost_at(m, 7, 1) == 86
        cells, n = path_of(m, (2, 1), 7, 1)
        assert n == 8 and path_sum(m, (2, 1), cells) == 86 and max(c[1] for c in cells) == 3
        assert int(m.pen[m.where(4, 0)]) == 5 and int(m.pen[m.where(4, 3)]) == 0
    out["penalty 0"] = case(strip(4), start, short, soft_d2=3, penalty=0)
    out["penalty 5"] = case(strip(4), start, long_, soft_d2=3, penalty=5)

    def on_penalised(m):
        assert cost_at(m, 4, 0) == 0 and cost_at(m, 5, 0) == 15 and ask(m, (2, 1), [(4, 0)])["next"][0] == 4
    out["a start on a penalised column"] = case(strip(4), [cell((2, 1), 4, 0)], on_penalised, soft_d2=3, penalty=5)

    def heavy(m):   # every column from u = 2 to u = 6 and the goal are within R = 3 of the pillar: six penalties at the least
        assert cost_at(m, 7, 1) == 78 + 6 * 65535
        cells, n = path_of(m, (2, 1), 7, 1)
        assert path_sum(m, (2, 1), cells) == 78 + 6 * 65535
    out["penalty 65535 without a budget"] = case(strip(3), start, heavy, gkw=dict(radius=3), soft_d2=10, penalty=65535, max_cost=0)
    # the same field under budgets at, one below and far above that cost: the compare against the budget at large values
    out["penalty 65535, the largest budget"] = case(strip(3), start, heavy, gkw=dict(radius=3), soft_d2=10, penalty=65535, max_cost=0xFFFFFFFF)
    out["penalty 65535, a budget that just holds"] = case(strip(3), start, heavy, gkw=dict(radius=3), soft_d2=10, penalty=65535,
                                                          max_cost=78 + 6 * 65535)

    def just_short(m):
        assert ask(m, (2, 1), [(7, 1), (0, 0)])["status"].tolist() == [1, 0] and cost_at(m, 7, 1) == NO
        assert m.info["max_cost_reached"] <= 78 + 6 * 65535 - 1
    out["penalty 65535, a budget one short"] = case(strip(3), start, just_short, gkw=dict(radius=3), soft_d2=10, penalty=65535,
                                                    max_cost=78 + 6 * 65535 - 1)
    return out


def budget():
    def expect(m):   # 10 max + 4 min <= 50
        assert m.info["n_reached"] == 24 and m.info["max_cost_reached"] == 50 and cost_at(m, 5, 0) == 50 and cost_at(m, 4, 3) == NO
        q = ask(m, (2, 1), [(4, 3), (4, 2)])
        assert q["status"].tolist() == [1, 0] and q["cost"].tolist() == [NO, 48] and q["metres"][0] == -1.0
        assert path_of(m, (2, 1), 4, 3)[1] == 0
    return case(terrain(np.zeros((8, 8))), [cell((2, 1), 0, 0)], expect, max_cost=50)


# 8 ---- a gap; a serpentine through 3 x 3 tiles
def gap():
    def expect(m):
        assert m.coords.tolist() == [[0, 0], [2, 0]] and m.info["n_reached"] == 64
        assert ask(m, (2, 1), [(16, 0), (8, 0), (7, 0)])["status"].tolist() == [1, 3, 0]
    return case(terrain(np.zeros((8, 24)), skip=[(1, 0)]), [cell((2, 1), 0, 0)], expect)


def serpentine(face):
    H = np.full((24, 24), WALL, np.int64)
    H[0::2] = 0
    for k, v in enumerate(range(1, 24, 2)):
        H[v, 23 if k % 2 == 0 else 0] = 0
    n = 12 * 24 + 12                                                    # twelve rows and a connector behind each

    def expect(m):
        assert m.info["n_traversable"] == m.info["n_reached"] == n and m.info["max_cost_reached"] == 10 * (n - 1)
        assert cost_at(m, -8, 7) == 10 * (n - 1) and path_of(m, (2, 1), -8, 7, max_len=5)[1] == n   # the grid's column (0, 23)
    return case(terrain(H, (-1, -2)), [cell((2, 1), -8, -16)], expect, face_connected=face)


# 9 ---- the int16 edge: every brick of int16_edge() solid floor, so every tile is ground through and through; a start in
# each brick at the edge.  A key that overflowed would make the brick int16_edge() calls lonely a neighbour, and the
# field would flow into it.
def edge(up, band):
    e = int16_edge()
    hdr, cells = e["hdr"], np.full_like(e["cells"], FLOOR)
    a, au, av = axes(up)
    lonely = {(b[au], b[av]) for b in e["lonely"]}
    started = {(int(s[au]) >> 3, int(s[av]) >> 3) for s in e["starts"]}

    def expect(m):
        tiles = [tuple(t) for t in m.coords.tolist()]
        assert len(tiles) >= 8 and m.info["n_traversable"] == 64 * len(tiles)
        n_started = 0
        for r, t in enumerate(tiles):
            if t in started:
                n_started += 1
                assert (m.cost[r] != NO).all(), t
            else:
                assert t in lonely and (m.cost[r] == NO).all(), t
        assert n_started >= 4 and m.info["n_reached"] == 64 * n_started

    return dict(hdr=hdr, cells=cells, gkw=dict(up=up, clearance=0, max_step=0, radius=4, support_labels=SUPPORT, **band), up=up,
                starts=np.asarray(e["starts"], np.int64).reshape(-1, 3), kw=dict(), expect=expect)


# 10 ---- boxes and starts
def boxes_and_starts():
    out = {}
    row, start = terrain(np.zeros((8, 24))), [cell((2, 1), 0, 0)]

    def boxed(m):
        assert m.coords.tolist() == [[0, 0], [1, 0]] and m.info["n_reached"] == 128 and ask(m, (2, 1), [(16, 0)])["status"][0] == 3
    out["a box"] = case(row, start, boxed, box=((0, -3), (1, 0)))

    def empty(m):
        assert len(m.coords) == 0 and m.cost.shape == (0, 64) and m.info["n_tiles"] == m.info["n_traversable"] == m.info["n_starts_used"] == 0
        assert ask(m, (2, 1), [(0, 0)])["status"][0] == 3 and path_of(m, (2, 1), 0, 0)[1] == 0
    out["the empty box"] = case(row, start, empty, box=((0, 0), (-1, 5)))
    H = np.full((16, 16), WALL, np.int64)                               # a corridor (0, 0) -> up -> across -> down to (15, 0)
    H[:, 0] = H[15, :] = H[:, 15] = 0

    def whole(m):
        assert cost_at(m, 15, 0) == 450

    def cut(m):
        assert m.coords.tolist() == [[0, 0], [1, 0]] and ask(m, (2, 1), [(15, 0), (0, 7), (0, 8)])["status"].tolist() == [1, 0, 3]
    out["a corridor"] = case(terrain(H), start, whole)
    out["a box that cuts a corridor"] = case(terrain(H), start, cut, box=((0, 0), (1, 0)))

    def nothing(m):
        assert m.info["n_starts_used"] == m.info["n_reached"] == m.info["max_cost_reached"] == 0 and (m.cost == NO).all()
        assert m.info["n_traversable"] == 23 and ask(m, (2, 1), [(0, 1)])["status"][0] == 1
    far = [cell((2, 1), 4, 1), cell((2, 1), 100, 100), [1 << 20, 0, 0], cell((2, 1), 0, 5)]       # the pillar, no tile, out of range, unseen
    out["no usable start"] = case(strip(3), far, nothing)

    def twice(m):
        assert m.info["n_starts_used"] == 1 and cost_at(m, 7, 1) == 78
    out["duplicate starts"] = case(strip(3), [cell((2, 1), 0, 1, 5), cell((2, 1), 0, 1, -900), cell((2, 1), 0, 1)], twice)

    def three(m):
        assert m.info["n_starts_used"] == 2 and cost_at(m, 0, 1) == cost_at(m, 7, 1) == 0 and cost_at(m, 3, 1) == 30
    out["three starts, one of them lethal"] = case(strip(3), [cell((2, 1), 0, 1), cell((2, 1), 4, 1), cell((2, 1), 7, 1)], three)
    return out


# 11 ---- the random archive: ground builds under three orientations and two flag sets, reach builds under every option
RANDOM_GROUNDS = [dict(up=up, clearance=1, max_step=6, radius=4, support_labels=SUPPORT, **band, **flags)
                  for up, band in (((2, 1), dict(h_lo=0, h_hi=12)), ((1, -1), dict(h_lo=-24, h_hi=6)), ((0, 1), dict(h_lo=-8, h_hi=20)))
                  for flags in (dict(unknown_passable=True), dict(unknown_passable=True, ignore_movable=True, none_is_lethal=True))]


def random_reaches():
    out = []
    for face, min_d2, penalty, max_cost in itertools.product((False, True), (0, 4), (0, 3), (0, 150)):
        out.append(dict(face_connected=face, min_d2=min_d2, soft_d2=9, penalty=penalty, max_climb=4, max_cost=max_cost))
    return out


def random_starts(ground, n=32):
    """world cells over the first ground columns (class 1, not lethal) of a ground answer"""
    a, au, av = axes((int(ground.o["up_axis"]), 1))
    out = []
    for r, (bu, bv) in enumerate(ground.coords.astype(np.int64).tolist()):
        for w in np.flatnonzero((ground.cells["cls"][r] & 11) == 1).tolist():
            g = [0, 0, 0]
            g[a], g[au], g[av] = 5, 8 * bu + (w & 7), 8 * bv + (w >> 3)
            out.append(g)
            if len(out) == n:
                return out
    return out


def sample_goals(m, up, n, seed):
    """world cells over reached, unreached and blocked columns of the field, and over columns of no tile"""
    rng = np.random.default_rng(seed)
    picks = [cell(up, 1000, 1000), cell(up, -9, 3)]
    for mask in (m.cost != NO, m.trav & (m.cost == NO), ~m.trav):
        at = np.argwhere(mask)
        if len(at):
            for r, w in at[rng.choice(len(at), min(n, len(at)), replace=False)].tolist():
                bu, bv = m.coords[r].astype(np.int64).tolist()
                picks.append(cell(up, 8 * bu + (w & 7), 8 * bv + (w >> 3), int(rng.integers(-50, 50))))
    return np.array(picks, np.int64)


def crafted():
    """name -> case, every crafted case (the random archive apart)"""
    out = {"one tile": one_tile(False), "one tile face": one_tile(True), "one tile at (-3, 2)": one_tile(False, (-3, 2)),
           "late corner": late_corner(), "budget": budget(), "gap": gap(), "serpentine": serpentine(False), "serpentine face": serpentine(True),
           "int16 edge z": edge((2, 1), dict(h_lo=0, h_hi=135)), "int16 edge x": edge((0, -1), dict(h_lo=-200, h_hi=-1)),
           "int16 edge y": edge((1, 1), dict(h_lo=0, h_hi=300))}
    for part in (seams(), climbs(), clearances(), penalties(), boxes_and_starts()):
        out.update(part)
    return out
