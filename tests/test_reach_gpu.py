"""The travel-cost field (sdm_reach_update / sdm_get_reach / sdm_query_reach / sdm_reach_paths) on the GPU against the
NumPy / heapq restatement in tests/reach_ref.py: the cost field, the info block (all but `rounds`), the query results and
the paths bit for bit, metres by its bit pattern, under both connectivities.  Crafted patterns on the map shapes of
tests/shape_cases.py (rings shifted on every axis), maps whose result arrays were filled by the real update, the shipped
grid with a budget; the rules for the starts, the budget and the clearance; goals on the host and on the device; the
snapshot rule, no side effects on the map, run-to-run identity and the argument checks.

Every case keeps its traversable (or, with a budget, its reachable) set at or below some 130 k cells, so that the Python
reference stays at seconds: on the large shapes the rest of the block is occupied."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import esdf_ref as er
from tests import parity_utils as pu
from tests import query_ref as qr
from tests import reach_ref as rr
from tests import shape_cases as sc
from tests.test_frontiers_gpu import crafted_map, snake_cells
from tests.test_instances_gpu import DRIVE, MAPS, get_map

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
NO = rr.NO_COST
BLOCK_CELLS = 131072   # the free sub-block of a crafted pattern holds at most this many cells
SNAKE_LINES = 64       # ... and a snake this many lines (32 full rows and their connectors)


def _dims(cfg):
    return np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.int64)


def word(N, c):
    c = np.asarray(c, np.int64)
    return c[..., 0] + N[0] * (c[..., 1] + N[1] * c[..., 2])


def sub_block(N):
    """the first cells of every axis that the pattern uses: the longest axis whole, the others halved until the block
    holds at most BLOCK_CELLS cells"""
    sub = N.copy()
    keep = int(np.argmax(N))
    for a in (2, 1, 0):
        while a != keep and sub.prod() > BLOCK_CELLS and sub[a] > 16:
            sub[a] //= 2
    assert sub.prod() <= BLOCK_CELLS
    return sub


def tile_corner_cells(N, sub):
    """the two cells either side of the first tile corner inside the block (the map's corner where an axis has one tile)"""
    t = np.where(sub > 8, 8, 1)
    return [tuple(t - 1), tuple(t)]


def pattern(name, kind):
    """-> (occ [z, y, x], start cells (x, y, z) rows)"""
    N = _dims(sc.config(name))
    sub = sub_block(N)
    occ = np.ones(tuple(N[::-1]), np.int8)
    blk = occ[:sub[2], :sub[1], :sub[0]]
    long_ax = int(np.argmax(N))
    if kind == "open":
        blk[:] = 0
        starts = [(0, 0, 0), tuple(sub // 2)]
    elif kind == "door":   # a wall across the longest axis with one free cell, the start in one corner, most cells behind the wall
        blk[:] = 0
        wall = [slice(None)] * 3
        wall[2 - long_ax] = sub[long_ax] // 2
        blk[tuple(wall)] = 1
        door = (sub - 1) // 2
        door[long_ax] = sub[long_ax] // 2
        blk[door[2], door[1], door[0]] = 0
        starts = [(0, 0, 0)]
    elif kind == "snake":   # one cell wide, everything else unknown: the longest dependent chain
        occ[:] = -1
        s = snake_cells(N)
        order = np.argsort(-N, kind="stable")
        s = s[s[:, int(order[1])] < SNAKE_LINES]
        occ[s[:, 2], s[:, 1], s[:, 0]] = 0
        starts = [tuple(s[0])]
    elif kind == "pinch":   # pairs of blocked cells that share an edge or a corner only: across a tile corner and at the map's faces
        blk[:] = 0
        a, b = [int(x) for x in np.argsort(-N, kind="stable")[:2]]
        t = np.where(sub > 8, 8, 1)
        mid = sub // 2
        for base in (t - 1, sub - 2, np.where(np.arange(3) == a, 0, t - 1)):
            p, q = mid.copy(), mid.copy()            # an edge-sharing pair in the plane of the two longest axes
            p[a], p[b], q[a], q[b] = base[a], base[b], base[a] + 1, base[b] + 1
            for c in (p, q):
                blk[c[2], c[1], c[0]] = 1
        for base in (t - 1, np.zeros(3, np.int64), sub - 2):   # corner-sharing pairs
            blk[base[2], base[1], base[0]] = 1
            blk[base[2] + 1, base[1] + 1, base[0] + 1] = 1
        first = np.argwhere(blk == 0)[0][::-1]
        starts = [tuple(first)]
    elif kind == "enclosed":
        blk[:] = 0
        c = sub // 2
        for d in np.vstack([np.eye(3, dtype=np.int64), -np.eye(3, dtype=np.int64)]):
            q = c + d
            blk[q[2], q[1], q[0]] = 1
        starts = [tuple(c)]
    elif kind == "random":   # 0.5 / 0.3 / 0.2 free / unknown / occupied over 32 cells per axis, the rest occupied
        r = np.minimum(N, 32)
        draw = np.random.default_rng(23 + ord(name)).choice(np.array([0, -1, 1], np.int8), size=tuple(r[::-1]), p=[0.5, 0.3, 0.2])
        occ[:r[2], :r[1], :r[0]] = draw
        rng = np.random.default_rng(5)
        starts = [tuple(rng.integers(0, r)) for _ in range(6)] + tile_corner_cells(N, r)
    else:
        raise KeyError(kind)
    return occ, np.array(starts, np.int64).reshape(-1, 3)


def check_build(cfg, g, geo, vox, starts, n_goals=192, seed=3, **kw):
    """build with start cell words `starts` under kw; field, info, origin, a sample of queries and paths against the
    restatement -> (cost, info, ref)"""
    g.reach_update(start_cells=starts, **kw)
    cost, info, origin = g.reach()
    ref = rr.field_of_map(geo, vox, starts, **kw)
    msg = rr.equal_all(cost, info, ref)
    assert msg is None, (kw, msg)
    assert np.array_equal(origin.view(np.uint32), (geo.center + geo.pmin).astype(np.float32).view(np.uint32))
    check_goals(cfg, g, geo, ref, n_goals, seed)
    return cost, info, ref


def sample_goals(ref, n, seed):
    """cell words: reached cells (the farthest among them), traversable unreached ones, others, and words outside the map"""
    rng = np.random.default_rng(seed)
    flat = ref.cost.ravel()
    reached = np.flatnonzero(flat != NO)
    parts = [rng.integers(0, flat.size + flat.size // 8, n // 4)]
    if len(reached):
        parts += [rng.choice(reached, n // 2), reached[np.argsort(flat[reached])[-8:]]]
    unreached = np.flatnonzero(ref.trav.ravel() & (flat == NO))
    if len(unreached):
        parts.append(rng.choice(unreached, n // 8))
    return np.concatenate(parts).astype(np.uint32)


def check_goals(cfg, g, geo, ref, n, seed, max_len=None):
    goals = sample_goals(ref, n, seed)
    got = g.query_reach(cells=goals)
    msg = rr.equal_results(got, ref.query(cfg["voxel_size"], cells=goals))
    assert msg is None, msg
    assert (got["pad"] == 0).all()
    want = ref.paths(cells=goals)
    longest = max(len(p) for p in want)
    max_len = max(longest, 1) if max_len is None else max_len
    rows, lens = g.reach_paths(cells=goals, max_len=max_len, fill=0xA5A5A5A5)
    assert np.array_equal(lens, [len(p) for p in want])
    for i, p in enumerate(want):
        k = min(len(p), max_len)
        assert np.array_equal(rows[i, :k], p[:k]) and (rows[i, k:] == 0xA5A5A5A5).all(), i
    return goals, got, want


# ---- crafted patterns on every map shape -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["open", "door", "snake", "pinch", "enclosed", "random"])
@pytest.mark.parametrize("name", sc.PARITY_CASES)
def test_map_shapes(name, kind):
    occ, starts = pattern(name, kind)
    cfg, g, geo, vox = crafted_map(name, occ)
    N = geo.N
    sw = word(N, starts)
    few = dict(n_goals=24) if kind == "snake" else {}   # (its paths are as long as the snake)
    for face in (False, True):
        if kind == "open":   # a start at a corner of the map, then one in the middle
            for s in sw:
                cost, info, ref = check_build(cfg, g, geo, vox, [s], face_connected=face)
                assert info["n_reached"] == info["n_traversable"] == (occ == 0).sum() and info["n_starts_used"] == 1
        elif kind == "random":
            for through in (False, True):
                cost, info, ref = check_build(cfg, g, geo, vox, sw, face_connected=face, through_unknown=through)
                assert info["n_traversable"] == ((occ == 0) | ((occ == -1) & through)).sum()
                assert 1 <= info["n_starts_used"] <= len(sw) and info["n_reached"] >= (8 if name == "A" else 100)
        else:
            cost, info, ref = check_build(cfg, g, geo, vox, sw, face_connected=face, **few)
            if kind == "door":   # the cells behind the wall are reached, through the door
                behind = np.argwhere(ref.cost != NO)[:, ::-1][:, int(np.argmax(N))].max()
                assert behind == sub_block(N)[int(np.argmax(N))] - 1 and info["n_reached"] == info["n_traversable"]
            elif kind == "snake":   # every cell of the snake, the last one at ten per cell
                assert info["n_reached"] == info["n_traversable"] == (occ == 0).sum()
                assert info["max_cost_reached"] == 10 * ((occ == 0).sum() - 1)
            elif kind == "pinch":
                assert info["n_reached"] == info["n_traversable"] or name == "A"
            elif kind == "enclosed":
                assert info["n_reached"] == 1 and info["n_starts_used"] == 1 and info["max_cost_reached"] == 0
    g.close()


def late_corner():
    """-> (occ [z, y, x] on shape B, start words, the words of c, f1, f2, d): a field on which a tile must wake the tile
    across its corner.  In the layer x = 1 a straight corridor of seven tiles brings start A's wave to c = (15, 55), the
    last cell of a tile, at cost 550 - round by round, because the tiles in the corridor's middle have no other reason to
    run.  The two face neighbours f1 = (16, 55) and f2 = (15, 56) of c, in the two tiles next to it, have had cost 560
    since the first round: each is the end of a serpentine of 55 moves that lies inside its own tile (through the layers
    x = 1 and x = 3) and has a start of its own.  So c's arrival lowers neither of them, neither of their tiles has a
    reason to wake the fourth tile, and its cell d = (16, 56), which stands at 570, must fall to 564 by the diagonal from c."""
    N = _dims(sc.config("B"))
    assert tuple(N) == (4, 32, 64)
    occ = np.ones(tuple(N[::-1]), np.int8)
    cells = [(1, 15, z) for z in range(56)] + [(1, 16, 55), (1, 15, 56), (1, 16, 56)]
    s1, s2 = [], []
    for i, y in enumerate((17, 19, 21, 23)):   # inside the tile y 16..23, z 48..55, from g1 = (17, 55) next to f1
        zs = list(range(55, 47, -1)) if i % 2 == 0 else list(range(48, 56))
        s1 += [(y, z) for z in zs] + ([(y + 1, zs[-1])] if i < 3 else [])
    for i, z in enumerate((57, 59, 61, 63)):   # inside the tile y 8..15, z 56..63, from g2 = (15, 57) next to f2
        ys = list(range(15, 7, -1)) if i % 2 == 0 else list(range(8, 16))
        s2 += [(y, z) for y in ys] + ([(ys[-1], z + 1)] if i < 3 else [])
    starts = []
    for s in (s1, s2):   # the layer x = 1, a connector in x = 2 at its end, and the same way back in the layer x = 3
        way = [(1,) + q for q in s] + [(2,) + s[-1]] + [(3,) + q for q in s[::-1]]
        cells += way
        starts.append(way[55])
    for x, y, z in cells:
        occ[z, y, x] = 0
    w = lambda c: int(word(N, c))  # noqa: E731
    return occ, [w((1, 15, 0))] + [w(q) for q in starts], [w((1, 15, 55)), w((1, 16, 55)), w((1, 15, 56)), w((1, 16, 56))]


def test_a_late_corner_needs_the_wake_up_across_it():
    occ, starts, (c, f1, f2, d) = late_corner()
    cfg, g, geo, vox = crafted_map("B", occ)
    cost, info, ref = check_build(cfg, g, geo, vox, starts)
    flat = ref.cost.ravel()
    assert (flat[c], flat[f1], flat[f2], flat[d]) == (550, 560, 560, 564) and info["n_starts_used"] == 3
    # without start A the cell d stands at 570: that is what a build that never woke d's tile again would leave
    assert rr.field_of_map(geo, vox, starts[1:]).cost.ravel()[d] == 570
    g.close()


# ---- starts -------------------------------------------------------------------------------------------------------------
def test_starts():
    occ, starts = pattern("B", "random")
    cfg, g, geo, vox = crafted_map("B", occ)
    N = geo.N
    free = np.flatnonzero((occ == 0).ravel())
    blocked = np.flatnonzero((occ == 1).ravel())
    several = free[[3, 500, 1000, 1500]]
    cost, info, ref = check_build(cfg, g, geo, vox, several)
    assert info["n_starts_used"] == 4 and (cost.ravel()[several] == 0).all()
    want = g.reach()[0].tobytes()
    # duplicates, an occupied cell, a word outside the map: the same field, the same count
    mixed = np.concatenate([several, several[:2], blocked[:3], [g.V, g.V + 17, 0xFFFFFFFF]]).astype(np.uint32)
    g.reach_update(start_cells=mixed)
    cost2, info2, _ = g.reach()
    assert cost2.tobytes() == want and info2["n_starts_used"] == 4
    # the same cells as points: their centres, plus points outside the map, NaN and infinity
    pts = np.concatenate([rr.cell_centres(geo, cfg["voxel_size"], mixed[:9]),
                          np.array([[1e6, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)])
    assert (rr.words_of_points(geo, pts)[:9] == mixed[:9]).all() and (rr.words_of_points(geo, pts)[9:] == NO).all()
    g.reach_update(starts=pts)
    cost3, info3, _ = g.reach()
    assert cost3.tobytes() == want and info3["n_starts_used"] == 4
    # no usable start: no error, every cell unreachable
    for kw in (dict(start_cells=blocked[:5]), dict(start_cells=np.zeros(0, np.uint32)), dict(starts=pts[9:])):
        g.reach_update(**kw)
        cost4, info4, _ = g.reach()
        assert (cost4 == NO).all() and info4["n_starts_used"] == 0 and info4["n_reached"] == 0 and info4["max_cost_reached"] == 0
        assert info4["n_traversable"] == len(free)
        q = g.query_reach(cells=np.concatenate([free[:50], blocked[:50]]))
        assert (q["status"][:50] == 1).all() and (q["status"][50:] == 2).all() and (q["cost"] == NO).all() and (q["next"] == 255).all()
        assert (g.reach_paths(cells=free[:50], max_len=4)[1] == 0).all()
    g.close()


# ---- the budget ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("face", [False, True])
def test_max_cost(face):
    occ, starts = pattern("D", "random")
    cfg, g, geo, vox = crafted_map("D", occ)
    sw = word(geo.N, starts[:2])
    full = rr.field_of_map(geo, vox, sw, face_connected=face, through_unknown=True)
    budget = 123
    cost, info, ref = check_build(cfg, g, geo, vox, sw, face_connected=face, through_unknown=True, max_cost=budget)
    assert np.array_equal(cost, np.where(full.cost <= budget, full.cost, NO))
    inside = (full.cost <= budget) & (full.cost > budget - 10)
    beyond = (full.cost > budget) & (full.cost <= budget + 10)
    assert inside.any() and beyond.any()   # cells just inside and just beyond the budget, or the case could not tell
    assert (cost[inside] != NO).all() and (cost[beyond] == NO).all() and info["max_cost_reached"] <= budget
    q = g.query_reach(cells=np.flatnonzero(beyond.ravel()).astype(np.uint32))
    assert (q["status"] == 1).all()
    g.close()


# ---- the clearance: the distance field's frame, not the current one ------------------------------------------------------
def test_clearance_reads_the_fields_snapshot():
    cfg, params, frames = synth.make_frames("T0", 8, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    assert g.L.sdm_reach_update(g.h, None, np.zeros(1, np.uint32).ctypes.data_as(C.c_void_p), 1, 4, 0, 0) == 1   # no field yet
    assert "sdm_esdf_update" in g.L.sdm_last_error().decode()
    for f in frames[:4]:
        g.update(*f)
    g.synchronize()
    geo_k, vox_k = qr.Geometry(cfg, g.ring_state()), g.voxels()
    g.esdf_update()
    for f in frames[4:7]:
        g.update(*f)
    g.synchronize()
    geo_n, vox_n = qr.Geometry(cfg, g.ring_state()), g.voxels()
    assert not np.array_equal(geo_k.eq, geo_n.eq) or not np.array_equal(geo_k.center, geo_n.center)
    kw = dict(through_unknown=True)
    trav_k = rr.traversable_of_field(er.snapshot_grid(geo_k, vox_k), er.edt_d2(er.obstacle_grid(geo_k, vox_k, cfg["max_movable_track"])), 4, True)
    cam = int(rr.words_of_points(geo_k, np.array([frames[3][2]], np.float32))[0])   # where the camera stood at frame k
    start = [start_for(trav_k, cam, False)]
    g.reach_update(start_cells=start, min_d2=4, **kw)
    cost, info, origin = g.reach()
    ref_k = rr.field_of_esdf(geo_k, vox_k, cfg["max_movable_track"], 0, start, 4, **kw)
    ref_n = rr.field_of_esdf(geo_n, vox_n, cfg["max_movable_track"], 0, start, 4, **kw)
    assert not np.array_equal(ref_k.cost, ref_n.cost)   # the two frames differ, so the case can tell
    msg = rr.equal_all(cost, info, ref_k)
    assert msg is None, msg
    assert info["n_reached"] >= 1000 and info["min_d2"] == 4
    assert info["n_traversable"] < rr.traversable(rr.occ_grid(geo_k, vox_k), True).sum()   # the clearance took cells away
    assert np.array_equal(origin.view(np.uint32), (geo_k.center + geo_k.pmin).astype(np.float32).view(np.uint32))
    check_goals(cfg, g, geo_k, ref_k, 192, 9)
    # points are taken in the field's frame as well
    pts = rr.cell_centres(geo_k, cfg["voxel_size"], np.flatnonzero(ref_k.cost.ravel() != NO)[:64])
    assert rr.equal_results(g.query_reach(xyz=pts), ref_k.query(cfg["voxel_size"], geo=geo_k, xyz=pts)) is None
    # without a clearance the same call reads the current frame
    cost, info, ref = check_build(cfg, g, geo_n, vox_n, start, **kw)
    assert info["min_d2"] == 0
    g.close()


# ---- real maps ------------------------------------------------------------------------------------------------------------
def nearest_traversable(trav, want_word):
    NZ, NY, NX = trav.shape
    cells = np.argwhere(trav)[:, ::-1]
    c0 = np.array([want_word % NX, (want_word // NX) % NY, want_word // (NX * NY)])
    near = cells[np.argmin(((cells - c0) ** 2).sum(axis=1))]
    return int(near[0] + NX * (near[1] + NY * near[2]))


def start_for(trav, want_word, face, min_reached=1000):
    """the start a real map's case uses: the wanted cell or, if it is not traversable, the traversable cell nearest to
    it; if that cell's component (the cells it reaches without a budget) has fewer than min_reached cells, the first
    cell of the largest component"""
    s = nearest_traversable(trav, want_word)
    label = rr.components(trav, face).ravel()
    roots, counts = np.unique(label[label >= 0], return_counts=True)
    if counts[roots == label[s]][0] >= min_reached:
        return s
    return int(roots[np.argmax(counts)])


REAL_VARIANTS = [dict(), dict(through_unknown=True, max_cost=250)]   # the observed free space alone; through the unknown, with a budget


@pytest.mark.parametrize("kind,name", MAPS)
def test_real_maps(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    cam = int(rr.words_of_points(geo, np.array([g.ring_state()["last_pos"]], np.float32))[0])
    assert cam != NO
    for face in (False, True):
        # (the free space alone on the driven maps, where the camera's frusta have swept far more than 1,000 cells free;
        # a map that began as a random dense state has no such space to speak of)
        for kw in (REAL_VARIANTS if kind == "driven" else REAL_VARIANTS[1:]):
            trav = rr.traversable(rr.occ_grid(geo, vox), kw.get("through_unknown", False))
            s = start_for(trav, cam, face)
            cost, info, ref = check_build(cfg, g, geo, vox, [s], face_connected=face, **kw)
            print(kind, name, "face" if face else "26", kw, "start", s, "camera", cam, dict(zip(info.dtype.names, info.tolist())))
            assert info["n_reached"] >= 1000


def test_shipped_grid_with_a_budget():
    cfg, params, frames = synth.make_frames("REF_ZED2_BOOST", 3)
    assert (cfg["x_n"], cfg["y_n"], cfg["z_n"]) == tuple(sc.config("F")[k] for k in ("x_n", "y_n", "z_n"))
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames:
        g.update(*f)
    g.synchronize()
    geo, vox = qr.Geometry(cfg, g.ring_state()), g.voxels()
    cam = np.array([g.ring_state()["last_pos"]], np.float32)
    trav = rr.traversable(rr.occ_grid(geo, vox), True)
    s = nearest_traversable(trav, int(rr.words_of_points(geo, cam)[0]))   # (through the unknown: whatever is no obstacle)
    for face in (False, True):
        cost, info, ref = check_build(cfg, g, geo, vox, [s], face_connected=face, through_unknown=True, max_cost=250)
        assert 1000 <= info["n_reached"] <= 200000 and info["n_reached"] < info["n_traversable"]
    g.close()


# ---- goals: host and device, short rows -----------------------------------------------------------------------------------
def test_queries_and_paths():
    cfg, g, geo, vox = get_map("driven", "C1")
    trav = rr.traversable(rr.occ_grid(geo, vox), True)
    cam = int(rr.words_of_points(geo, np.array([g.ring_state()["last_pos"]], np.float32))[0])
    s = start_for(trav, cam, False)
    g.reach_update(start_cells=[s], through_unknown=True, max_cost=250)
    ref = rr.field_of_map(geo, vox, [s], through_unknown=True, max_cost=250)
    assert rr.equal_all(*g.reach()[:2], ref) is None
    # 4,096 goals as points: everywhere in and round the map, on reached cells, on blocked cells, NaN and infinity among them
    rng = np.random.default_rng(77)
    size, N = np.float32(cfg["voxel_size"]), geo.N
    lo, hi = geo.center + geo.pmin, geo.center + geo.pmin + N.astype(np.float32) * size
    pts = rng.uniform(lo - 2 * size, hi + 2 * size, (4096, 3)).astype(np.float32)
    reached = np.flatnonzero(ref.cost.ravel() != NO)
    pts[:2048] = rr.cell_centres(geo, size, rng.choice(reached, 2048)) + rng.uniform(-0.45, 0.45, (2048, 3)).astype(np.float32) * size
    blocked = np.flatnonzero(~trav.ravel())
    pts[2048:2112] = rr.cell_centres(geo, size, rng.choice(blocked, 64)) + rng.uniform(-0.45, 0.45, (64, 3)).astype(np.float32) * size
    pts[4000:4004] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]]
    want = ref.query(size, geo=geo, xyz=pts)
    assert all((want["status"] == k).sum() >= 4 for k in (0, 1, 3)) and (want["status"] == 0).sum() >= 2048
    assert (want["status"] == 2).sum() >= 64
    host = g.query_reach(xyz=pts)
    msg = rr.equal_results(host, want)
    assert msg is None, msg
    words = rr.words_of_points(geo, pts).astype(np.uint32)
    assert rr.equal_results(g.query_reach(cells=words), want) is None   # the same goals as cell words
    # the paths of a sample against the restatement, all of them host against device; rows shorter than some paths
    lens_ref = np.array([len(p) for p in ref.paths(cells=words[:512])])
    full = int(lens_ref.max())
    assert full >= 12
    short = full // 2
    for max_len in (full, short, 0):
        rows, lens = g.reach_paths(xyz=pts, max_len=max_len, fill=0xA5A5A5A5)
        assert np.array_equal(lens[:512], lens_ref) and (lens[want["status"] != 0] == 0).all() and (lens[want["status"] == 0] >= 1).all()
        for i, p in enumerate(ref.paths(cells=words[:512])):
            k = min(len(p), max_len)
            assert np.array_equal(rows[i, :k], p[:k]) and (rows[i, k:] == 0xA5A5A5A5).all(), (max_len, i)
        if max_len == short:
            assert (lens > short).any() and ((lens > 0) & (lens < short)).any()
        # device mode: the same bytes, the sentinel behind every path
        d_pts, d_rows, d_lens = g.device_put(pts), g.device_put(np.full((4096, max(max_len, 1)), 0xA5A5A5A5, np.uint32)), g.device_alloc(4096 * 4)
        g.reach_paths(xyz=d_pts, n=4096, max_len=max_len, on_device=True, cells_out=d_rows, len_out=d_lens)
        g.synchronize()
        assert np.array_equal(g.device_download(d_lens, 4096 * 4, np.int32), lens)
        if max_len:
            assert np.array_equal(g.device_download(d_rows, 4096 * max_len * 4, np.uint32).reshape(4096, max_len), rows)
        for p in (d_pts, d_rows, d_lens):
            g.device_free(p)
    d_pts, d_words, d_out = g.device_put(pts), g.device_put(words), g.device_alloc(4096 * 16)
    for kw in (dict(xyz=d_pts), dict(cells=d_words)):
        g.reach_update(start_cells=[s], through_unknown=True, max_cost=250)   # (in between: the query reads the new build)
        g.query_reach(n=4096, out=d_out, on_device=True, **kw)
        g.synchronize()
        assert g.device_download(d_out, 4096 * 16, binding.REACH_RESULT).tobytes() == host.tobytes()
    for p in (d_pts, d_words, d_out):
        g.device_free(p)


# ---- the snapshot rule, side effects, run to run, a second build, arguments ------------------------------------------------
def test_snapshot_and_stream_order():
    """Build after frame k, then two more frames (ring shifts) and a clear, nothing synchronised in between: field,
    queries and paths are frame k's.  A new build gives the new frame's."""
    cfg, params, frames = synth.make_frames("T0", 8, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames[:4]:
        g.update(*f)
    g.synchronize()
    geo_k, vox_k = qr.Geometry(cfg, g.ring_state()), g.voxels()
    trav = rr.traversable(rr.occ_grid(geo_k, vox_k), True)
    cam = np.array([g.ring_state()["last_pos"]], np.float32)
    s = start_for(trav, int(rr.words_of_points(geo_k, cam)[0]), False)
    g.reach_update(start_cells=[s], through_unknown=True)
    for f in frames[4:6]:
        g.update(*f)
    g.clear()
    cost, info, origin = g.reach()
    ref = rr.Field(trav, [s], through_unknown=True)
    assert rr.equal_all(cost, info, ref) is None and info["n_reached"] >= 1000
    assert np.array_equal(origin, (geo_k.center + geo_k.pmin).astype(np.float32))
    check_goals(cfg, g, geo_k, ref, 192, 4)
    pts = rr.cell_centres(geo_k, cfg["voxel_size"], np.flatnonzero(ref.cost.ravel() != NO)[::97])
    assert rr.equal_results(g.query_reach(xyz=pts), ref.query(cfg["voxel_size"], geo=geo_k, xyz=pts)) is None   # (frame k's geometry)
    g.update(*frames[6])
    g.synchronize()
    geo_n, vox_n = qr.Geometry(cfg, g.ring_state()), g.voxels()
    cost, info, new = check_build(cfg, g, geo_n, vox_n, [s], through_unknown=True, face_connected=True)
    assert not np.array_equal(new.cost, ref.cost)
    g.close()


def test_reach_leaves_the_map_alone():
    cfg, params, frames = synth.make_frames("T0", 6, n_dynamic=2)
    a = binding.SdmMap(cfg, params, synth.noise_table())
    b = binding.SdmMap(cfg, params, synth.noise_table())
    goals = np.arange(0, b.V, 37, dtype=np.uint32)
    for i, f in enumerate(frames):
        a.update(*f)
        b.update(*f)
        b.reach_update(start_cells=goals[::5], face_connected=bool(i & 1), through_unknown=True, max_cost=200 * (i & 2))
        b.query_reach(cells=goals)
        b.reach_paths(cells=goals, max_len=8)
    a.synchronize()
    b.synchronize()
    rep = pu.compare_maps(a, b, a.S, check_results=True)
    assert not rep, "\n".join(rep)
    assert np.array_equal(a.voxels().view(np.uint64), b.voxels().view(np.uint64))
    for m in (a, b):
        m.esdf_update()
        m.frontiers_update()
    for x, y in zip(a.esdf()[:2], b.esdf()[:2]):
        assert np.array_equal(x, y)
    assert a.frontiers()[0].tobytes() == b.frontiers()[0].tobytes()
    a.close()
    b.close()


def test_run_to_run_and_a_second_build():
    cfg, g, geo, vox = get_map("dense", "C1")
    trav = rr.traversable(rr.occ_grid(geo, vox), True)
    s = start_for(trav, int(np.flatnonzero(trav.ravel())[trav.sum() // 2]), False)
    runs = []
    for _ in range(2):
        g.reach_update(start_cells=[s], through_unknown=True, max_cost=250)
        cost, info, _ = g.reach()
        q = g.query_reach(cells=np.arange(0, g.V, 11, dtype=np.uint32))
        runs.append((cost.tobytes(), q.tobytes(), tuple(info.tolist()[:4]) + tuple(info.tolist()[5:])))
    assert runs[0] == runs[1]
    # other flags, another start, no budget: nothing of the first build is left
    other = int(np.flatnonzero((occ := rr.occ_grid(geo, vox)).ravel() == 0)[5])
    cost, info, ref = check_build(cfg, g, geo, vox, [other], face_connected=True)
    assert cost.tobytes() != runs[0][0] and info["flags"] == 1 and info["max_cost"] == 0
    assert (cost[occ != 0] == NO).all()


def test_argument_errors():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    L, INV = g.L, 1
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cells, pts = np.zeros(4, np.uint32), np.zeros((4, 3), np.float32)
    out, rows, lens = np.zeros(4, binding.REACH_RESULT), np.zeros((4, 8), np.uint32), np.zeros(4, np.int32)
    info = np.zeros(1, binding.REACH_INFO)
    # before any build
    assert L.sdm_get_reach(g.h, None, vp(info), None) == INV and "sdm_reach_update" in L.sdm_last_error().decode()
    assert L.sdm_query_reach(g.h, None, vp(cells), 4, vp(out), 0) == INV and "sdm_reach_update" in L.sdm_last_error().decode()
    assert L.sdm_reach_paths(g.h, None, vp(cells), 4, 8, vp(rows), vp(lens), 0) == INV
    for call in (g.reach, lambda: g.query_reach(cells=cells), lambda: g.reach_paths(cells=cells, max_len=4)):
        with pytest.raises(binding.SdmError):
            call()
    # the build's arguments
    assert L.sdm_reach_update(g.h, None, None, 0, 0, 0, 0) == INV            # no start pointer
    assert L.sdm_reach_update(g.h, vp(pts), vp(cells), 4, 0, 0, 0) == INV    # both
    assert L.sdm_reach_update(g.h, None, vp(cells), -1, 0, 0, 0) == INV
    assert L.sdm_reach_update(g.h, None, vp(cells), 4, 0, 0, 0x4) == INV
    assert L.sdm_reach_update(g.h, None, vp(cells), 4, 0, 0, 0x80000000) == INV
    assert L.sdm_reach_update(g.h, None, vp(cells), 4, 1, 0, 0) == INV        # a clearance without a distance field
    assert L.sdm_reach_update(g.h, None, vp(cells), 0, 0, 0, 0) == 0          # no starts: no error
    assert L.sdm_reach_update(g.h, None, vp(cells), 4, 0, 0, 0x3) == 0
    assert L.sdm_get_reach(g.h, None, None, None) == 0 and L.sdm_get_reach(g.h, None, vp(info), None) == 0
    assert info[0]["flags"] == 3 and info[0]["n_traversable"] == g.V and info[0]["n_reached"] == g.V   # a fresh map, through the unknown
    # the queries' arguments
    assert L.sdm_query_reach(g.h, None, None, 4, vp(out), 0) == INV
    assert L.sdm_query_reach(g.h, vp(pts), vp(cells), 4, vp(out), 0) == INV
    assert L.sdm_query_reach(g.h, None, vp(cells), -1, vp(out), 0) == INV
    assert L.sdm_query_reach(g.h, None, vp(cells), 4, None, 0) == INV
    assert L.sdm_query_reach(g.h, None, vp(cells), 4, vp(out), 0x2) == INV
    assert L.sdm_query_reach(g.h, None, vp(cells), 0, vp(out), 0) == 0
    assert L.sdm_query_reach(g.h, None, vp(cells), 4, vp(out), 0) == 0 and (out["status"] == 0).all()
    assert L.sdm_reach_paths(g.h, None, None, 4, 8, vp(rows), vp(lens), 0) == INV
    assert L.sdm_reach_paths(g.h, vp(pts), vp(cells), 4, 8, vp(rows), vp(lens), 0) == INV
    assert L.sdm_reach_paths(g.h, None, vp(cells), 4, -1, vp(rows), vp(lens), 0) == INV
    assert L.sdm_reach_paths(g.h, None, vp(cells), -1, 8, vp(rows), vp(lens), 0) == INV
    assert L.sdm_reach_paths(g.h, None, vp(cells), 4, 8, None, vp(lens), 0) == INV
    assert L.sdm_reach_paths(g.h, None, vp(cells), 4, 8, vp(rows), None, 0) == INV
    assert L.sdm_reach_paths(g.h, None, vp(cells), 4, 8, vp(rows), vp(lens), 0x4) == INV
    assert L.sdm_reach_paths(g.h, None, vp(cells), 4, 0, None, vp(lens), 0) == 0 and (lens == 1).all()   # (cell 0 is a start)
    assert L.sdm_reach_paths(g.h, None, vp(cells), 4, 8, vp(rows), vp(lens), 0) == 0
    g.close()
    s = binding.SdmMap(cfg, PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert s.L.sdm_reach_update(s.h, None, vp(cells), 4, 0, 0, 0) == INV and "shard" in s.L.sdm_last_error().decode()
    assert s.L.sdm_get_reach(s.h, None, vp(info), None) == INV
    assert s.L.sdm_query_reach(s.h, None, vp(cells), 4, vp(out), 0) == INV
    assert s.L.sdm_reach_paths(s.h, None, vp(cells), 4, 8, vp(rows), vp(lens), 0) == INV
    with pytest.raises(binding.SdmError):
        s.reach_update(start_cells=cells)
    s.close()
