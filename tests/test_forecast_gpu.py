"""The forecast (sdm_forecast_update / sdm_get_forecast / sdm_get_forecast_cells / sdm_query_forecast /
sdm_query_forecast_segments) on the GPU against the NumPy restatement in tests/forecast_ref.py: both field arrays, the info
block, the origin, the cell list and 4,096 point-time queries bit for bit; space-time segments exactly but for t (the
segment query's tolerance), on the segments that are ambiguous neither in space nor in time.  Crafted scenes on the map
shapes of tests/shape_cases.py (rings shifted on every axis), maps whose result arrays were filled by the real update;
the snapshot rule in stream order, no side effects on the map, run-to-run identity, host against device mode and the
argument checks."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import forecast_ref as fc
from tests import parity_utils as pu
from tests import query_ref as qr
from tests import shape_cases as sc
from tests.test_instances_gpu import DRIVE, MAPS, get_map

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
SHAPES = ["A", "B", "C", "D", "F"]
T_LINE, T_DOT, T_STAYS, T_WRAP, T_TWIN, T_CLOUD, T_ABSENT = 1, 2, 3, 4, 5, 6, 77   # T_STAYS is never given a motion, T_ABSENT owns no cell
HORIZONS = np.array([0.25, 0.5, 1.0, 2.0, 4.0], np.float32)
SEG_EXCLUDED_MAX = 0.12
_SCENES = {}


def unit(a, k=1):
    e = np.zeros(3, np.int64)
    e[a] = k
    return e


def scene_cells(N, wrap):
    """-> {(x, y, z): track}, unknown cells, the guessed cell: a line of up to five cells along the longest axis from the
    origin corner (its second cell a guessed birth), a dot in the far corner and a twin two cells before it, a movable
    track that is never given a motion, an object of six cells either side of the ring's wrap point on every axis, a
    building and an unknown cell in the middle; on maps of more than 64 cells a sprinkle of a moving cloud, buildings and
    unknown cells over the first 24 cells of every axis"""
    a = int(np.argmax(N))
    far = N - 1
    cells, unknown = {}, []
    if N.prod() > 64:
        rng = np.random.default_rng(int(N.prod()))
        sub = np.minimum(N, 24)
        draw = rng.random(tuple(sub))
        for c in np.argwhere(draw < 0.03):
            cells[tuple(int(v) for v in c)] = T_CLOUD
        for c in np.argwhere((draw >= 0.03) & (draw < 0.05)):
            cells[tuple(int(v) for v in c)] = synth.TRACK_BUILDING
        unknown = [tuple(int(v) for v in c) for c in np.argwhere((draw >= 0.05) & (draw < 0.10))]
    special = {}
    for i in range(min(int(N[a]), 5)):
        special[tuple(unit(a, i))] = T_LINE
    special[tuple(far)] = T_DOT
    special[tuple(far - unit(a, 2))] = T_TWIN
    special[(0, int(far[1]), int(far[2]))] = T_STAYS
    for ax in range(3):
        for c in (wrap[ax] - 1, wrap[ax]):
            cell = N // 3
            cell[ax] = c % N[ax]
            special[tuple(int(v) for v in cell)] = T_WRAP
    special[tuple(N // 2)] = synth.TRACK_BUILDING
    middle_unknown = tuple(int(v) for v in N // 2 + unit(a))
    keep_free = {tuple(int(v) for v in far - unit(a))}   # where the dot and its twin meet
    cells = {c: t for c, t in cells.items() if c not in keep_free and c != middle_unknown}
    cells.update({tuple(int(v) for v in c): t for c, t in special.items()})
    unknown = [c for c in unknown if c not in cells and c not in keep_free] + [middle_unknown]
    assert middle_unknown not in cells and len(set(special.values())) == 6
    return cells, unknown, tuple(unit(a, 1))


def scene(name):
    """the crafted map of shape `name` (made once): the state is loaded on a ring shifted on every axis, one frame that
    sees nothing writes every result -> cfg, map, geometry, voxels, (occ, track) grids"""
    if name not in _SCENES:
        cfg = sc.config(name)
        ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
        geo0 = qr.Geometry(cfg, ring)
        N = geo0.N
        cells, unknown, guessed = scene_cells(N, (N - geo0.eq) % N)
        occupied = np.array(sorted(cells), np.int64)
        tracks = np.array([cells[tuple(c)] for c in occupied], np.uint16)
        labels = np.where(tracks <= cfg["max_movable_track"], synth.LABEL_CAR, synth.LABEL_BUILDING).astype(np.uint8)
        st = sc.crafted_state(cfg, ring, occupied, np.array(unknown, np.int64), tracks, labels)
        # the guessed birth: a particle below the occupancy threshold whose status says it was guessed (occ == 2)
        S = 1 << cfg["p_n"]
        gi = int(geo0.voxel(np.array([guessed]))[0]) * S + 1
        st["status"][gi], st["w"][gi] = 3, 0.3
        g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
        g.load_state(st)
        g.set_ring_state(ring)
        depth = np.full((cfg["height"], cfg["width"]), np.nan, np.float32)
        cloud = np.zeros(cfg["height"] * cfg["width"], synth.LABELED_POINT)
        g.update(depth, cloud, np.array(ring["last_pos"], np.float32), synth.yaw_quat(0.0).astype(np.float32), None, sync=True)
        got = g.ring_state()
        assert got["eq_steps"] == ring["eq_steps"] and got["map_center"] == ring["map_center"]
        geo, vox = qr.Geometry(cfg, got), g.voxels()
        assert all(e != 0 for e in geo.eq)
        occ, track = fc.grids(geo, vox)
        want = np.zeros(occ.shape, np.int8)
        for c in unknown:
            want[c[2], c[1], c[0]] = -1
        want[occupied[:, 2], occupied[:, 1], occupied[:, 0]] = 1
        assert np.array_equal(np.minimum(occ, 1), want)
        assert np.array_equal(track[occupied[:, 2], occupied[:, 1], occupied[:, 0]], tracks)
        assert occ[guessed[2], guessed[1], guessed[0]] == 2 and track[guessed[2], guessed[1], guessed[0]] == T_LINE   # an occ == 2 source
        _SCENES[name] = (cfg, g, geo, vox, (occ, track))
    return _SCENES[name]


def per_second(cfg, cells):
    """the velocity that moves `cells` cells a second (t = 1: v * t / size is the whole number or next to it)"""
    return (np.asarray(cells, np.float64) * np.float64(np.float32(cfg["voxel_size"]))).astype(np.float32)


def sample_points(geo, size, ref, n, seed):
    """n point-times: all over the block and two cells round it, half of them on marked, source and unknown cells; times
    from 0 to beyond the last horizon, some exactly on a horizon; NaN and infinity among them"""
    rng = np.random.default_rng(seed)
    lo, hi = geo.center + geo.pmin, geo.center + geo.pmin + geo.N.astype(np.float32) * size
    p = np.empty((n, 4), np.float32)
    p[:, :3] = rng.uniform(lo - 2 * size, hi + 2 * size, (n, 3))
    cls = (ref.mask.ravel() >> 16) & 3
    pool = np.flatnonzero(((ref.mask.ravel() & 0xFFFF) != 0) | (cls != 1))
    if len(pool):
        w = rng.choice(pool, n // 2).astype(np.int64)
        c = np.stack([w % geo.N[0], (w // geo.N[0]) % geo.N[1], w // (geo.N[0] * geo.N[1])], 1)
        p[:n // 2, :3] = lo + (c.astype(np.float32) + rng.uniform(0.1, 0.9, (n // 2, 3)).astype(np.float32)) * size
    p[:, 3] = rng.uniform(0, 1.25 * float(ref.t[-1]), n)
    p[::7, 3] = rng.choice(ref.t, len(p[::7]))
    p[5], p[6], p[12], p[13] = [np.nan, 0, 0, 1], [0, 0, np.inf, 1], [lo[0], lo[1], lo[2], np.nan], [lo[0], lo[1], lo[2], np.inf]
    return p


def check_build(cfg, g, geo, vox, mo, horizons, swept=False, occ_track=None, seed=1):
    """one build against the restatement: field, info, origin, cell list, 4,096 point-time queries -> (mask, first, info, ref)"""
    g.forecast_update(mo, horizons, swept)
    mask, first, info, origin = g.forecast()
    ref = fc.Field(geo, vox, cfg["voxel_size"], mo, horizons, swept, occ_track=occ_track)
    msg = fc.equal_fields(mask, first, info, ref)
    assert msg is None, msg
    assert np.array_equal(origin.view(np.uint32), (geo.center + geo.pmin).astype(np.float32).view(np.uint32))
    cell, cm, cf = g.forecast_cells()
    want = ref.cells()
    assert np.array_equal(cell, want[0]) and np.array_equal(cm, want[1]) and np.array_equal(cf, want[2])
    if len(cell) > 1:   # a short list: its head, the true count
        k = len(cell) // 2
        c2, m2, f2, total = g.forecast_cells(cap=k)
        assert total == len(cell) and np.array_equal(c2, cell[:k]) and np.array_equal(m2, cm[:k]) and np.array_equal(f2, cf[:k])
    pts = sample_points(geo, np.float32(cfg["voxel_size"]), ref, 4096, seed)
    got = g.query_forecast(pts)
    msg = fc.equal_records(got, ref.query(pts), ("state", "horizon", "track", "mask", "first_horizon", "pad"))
    assert msg is None, msg
    return mask, first, info, ref


# ---- crafted scenes on every map shape ------------------------------------------------------------------------------------
def case_motions(case, cfg, N):
    """-> (motions, horizons, swept) of a crafted case on a map of N cells"""
    a = int(np.argmax(N))
    line = min(int(N[a]), 5)
    v = lambda cells: per_second(cfg, cells)  # noqa: E731
    absent = (T_ABSENT, v([1, 1, 1]))
    wrap, cloud = (T_WRAP, v([1, -1, 1])), (T_CLOUD, v([-1, 2, 0]))
    if case == "plus_x":
        return [(T_LINE, v([1, 0, 0])), wrap, absent], [1, 2, 3], False
    if case == "minus_y":
        return [(T_LINE, v([0, -1, 0])), (T_STAYS + 100, v([0, 0, 0])), wrap, cloud], [0.5, 1, 2.5], False
    if case == "diagonal":
        return [(T_LINE, v([1, 1, 1])), (T_WRAP, v([-1, -1, -1])), cloud], [1, 2, 3, 4], False
    if case == "last_cell_and_beyond":   # the line's last cell lands on cell N - 1, then on N: lost
        return [(T_LINE, v(unit(a)))], [max(int(N[a]) - line, 0.25), int(N[a]) - line + 1], False
    if case == "onto_itself":
        return [(T_LINE, v(unit(a))), absent], [1], False
    if case == "same_cell_same_horizon":   # the twin and the dot meet between them: the smaller track is first
        return [(T_TWIN, v(unit(a))), (T_DOT, v(-unit(a)))], [1, 2], False
    if case == "same_cell_other_horizon":  # the twin arrives at horizon 0, the dot (half as fast) at horizon 1: the earlier one is first
        return [(T_TWIN, v(unit(a))), (T_DOT, v(-unit(a)) * np.float32(0.5))], [1, 2], False
    if case == "onto_building_and_unknown":
        return [(T_DOT, v(N // 2 - (N - 1))), (T_TWIN, v(N // 2 + unit(a) - (N - 1 - unit(a, 2))))], [1], False
    if case == "sixteen_horizons":
        slow = np.float32(0.25)   # two cells at the last horizon: bit 15 also on the smallest map
        return [(T_LINE, v(unit(a)) * slow), (T_WRAP, wrap[1] * slow), (T_CLOUD, cloud[1] * slow)], np.arange(1, 17) * 0.5, False
    if case == "swept_40":   # a 40-cell step within one horizon, then 20 more
        return [(T_DOT, v(-40 * unit(a) + 7 * unit((a + 1) % 3, -1))), (T_LINE, v(40 * unit(a))), wrap], [1, 1.5], True
    if case == "swept_cloud":
        return [cloud, wrap, (T_LINE, v([3, 2, -1]))], HORIZONS, True
    if case == "no_motions":
        return [], HORIZONS, False
    raise KeyError(case)


CASES = ["plus_x", "minus_y", "diagonal", "last_cell_and_beyond", "onto_itself", "same_cell_same_horizon", "same_cell_other_horizon",
         "onto_building_and_unknown", "sixteen_horizons", "swept_40", "swept_cloud", "no_motions"]


def run_case(name, case):
    cfg, g, geo, vox, ot = scene(name)
    N = geo.N
    a = int(np.argmax(N))
    table, horizons, swept = case_motions(case, cfg, N)
    mo = fc.motions([t for t, _ in table], [w for _, w in table]) if table else None
    mask, first, info, ref = check_build(cfg, g, geo, vox, mo, horizons, swept, occ_track=ot, seed=len(case))
    occ, track = ot
    word = lambda c: int(c[0] + N[0] * (c[1] + N[1] * c[2]))  # noqa: E731
    flat_m, flat_f = mask.ravel(), first.ravel()
    in_table = set(t for t, _ in table)
    # what is never given a motion stays; a guessed-occupied cell of a moving track is a source; the building and the unknown cell
    assert (flat_m[word((0, N[1] - 1, N[2] - 1))] >> 16) == 2 and (flat_m[word(N // 2)] >> 16) == 2 and (flat_m[word(N // 2 + unit(a))] >> 16) == 0
    assert (flat_m[word(unit(a))] >> 16) == (3 if T_LINE in in_table else 2) and occ[tuple(unit(a)[::-1])] == 2
    assert info["n_motions"] == len(table) and info["n_horizons"] == len(horizons) and info["flags"] == int(swept)
    meet = N - 1 - unit(a)
    if case == "last_cell_and_beyond":
        line = min(int(N[a]), 5)
        assert flat_m[word(unit(a, int(N[a]) - 1))] & 1 and info["n_marks_out"] == 1 and info["n_marks_in"] == 2 * line - 1
    elif case == "onto_itself":
        assert (flat_m[word(unit(a))] & 0x3FFFF) == (3 << 16 | 1) and flat_f[word(unit(a))] == T_LINE
        assert info["n_marks_out"] == (1 if N[a] <= 5 else 0)   # (the line's last cell leaves a map as short as the line)
    elif case == "same_cell_same_horizon":
        assert (flat_m[word(meet)] & 0xFFFF) == 1 and flat_f[word(meet)] == T_DOT and info["n_marks_in"] + info["n_marks_out"] == 4
    elif case == "same_cell_other_horizon":
        assert (flat_m[word(meet)] & 0xFFFF) == 3 and flat_f[word(meet)] == T_TWIN and flat_f[word(N - 1)] == T_DOT
    elif case == "onto_building_and_unknown":
        assert flat_m[word(N // 2)] == (2 << 16 | 1) and flat_m[word(N // 2 + unit(a))] == 1
        q = ref.query(np.array([list((geo.center + geo.pmin) + (c + 0.5) * np.float32(cfg["voxel_size"])) + [0.5] for c in (N // 2, N // 2 + unit(a))]))
        assert q["state"].tolist() == [1, 2]   # the building stays whatever lands on it; the unknown cell is predicted
    elif case == "sixteen_horizons":
        assert (flat_m >> 15 & 1).any() and info["n_stamps"] == 48
    elif case == "swept_40":
        assert info["n_stamps"] == 60 + 60 + 2 and (N[a] < 64 or info["n_marks_in"] > 60)
    elif case == "no_motions":
        assert info["n_sources"] == 0 and info["n_marked"] == 0 and info["n_stamps"] == 0 and (first == fc.NOTHING).all()
        assert np.array_equal(mask >> 16, np.where(occ == -1, 0, np.where(occ == 0, 1, 2)))
    if T_WRAP in in_table:   # the object either side of the wrap point of every axis moves as one
        assert info["n_sources"] >= 5


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", SHAPES)
def test_crafted_scenes(name, case):
    run_case(name, case)


def test_the_largest_shape():
    run_case("E", "swept_cloud")


# ---- maps filled by the real update ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", MAPS)
def test_real_maps(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    g.instances_update(movable_only=True)
    table, _ = g.instances()
    tracks = table["track"][:64]
    rng = np.random.default_rng(len(tracks) + 3)
    mo = fc.motions(tracks, rng.normal(0, 1.5, (len(tracks), 3))) if len(tracks) else None
    ot = fc.grids(geo, vox)
    for swept in (False, True):
        mask, first, info, ref = check_build(cfg, g, geo, vox, mo, HORIZONS, swept, occ_track=ot, seed=9)
        print(kind, name, "swept" if swept else "plain", dict(zip(info.dtype.names, info.tolist())))
        if len(tracks):
            assert info["n_sources"] > 0 and info["n_marked"] > 0


# ---- space-time segments --------------------------------------------------------------------------------------------------
def random_segments(geo, size, n=4000, seed=7):
    rng = np.random.default_rng(seed)
    lo, hi = geo.center + geo.pmin - 2 * size, geo.center + geo.pmin + (geo.N.astype(np.float32) + 2) * size
    a = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    b = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    short = np.arange(n) % 2 == 1
    b[short] = a[short] + rng.normal(0, 3 * size, (int(short.sum()), 3)).astype(np.float32)
    ta = rng.uniform(0, 3, n).astype(np.float32)
    tb = (ta + rng.uniform(0, 2, n).astype(np.float32)).astype(np.float32)
    return np.concatenate([a, ta[:, None], b, tb[:, None]], axis=1)


def hand_segments(geo, size):
    lo = geo.center + geo.pmin
    mid = lo + ((geo.N // 2).astype(np.float32) + np.array([0.37, 0.21, 0.68], np.float32)) * size
    far = lo + (geo.N.astype(np.float32) + 5) * size
    out = lo - 5 * size
    near = lo + np.array([0.3, 0.45, 0.6], np.float32) * size
    rows = [list(mid) + [1.1] + list(mid) + [2.1],                       # zero length
            list(far) + [0.0] + list(far + size) + [1.0],                # entirely outside
            list(out) + [0.0] + list(mid) + [3.7],                       # entering from outside
            list(near) + [1.5] + list(mid) + [1.5],                      # ta == tb
            list(mid) + [2.0] + list(near) + [1.0],                      # ta > tb
            [np.nan] + list(mid[1:]) + [0.0] + list(mid) + [1.0],
            list(mid) + [np.nan] + list(lo) + [1.0],
            list(mid) + [0.0] + list(lo) + [np.inf]]
    return np.array(rows, np.float32)


def check_segments(geo, ref, seg, got, flags):
    want = ref.query_segments(seg, **flags)
    ok = ~qr.segment_ambiguous(geo, seg[:, 0:3], seg[:, 4:7]) & ~want["time_ambiguous"]
    for k in ("cell", "cells", "state", "horizon", "track"):
        bad = np.flatnonzero(ok & (got[k] != want[k]))
        assert not len(bad), (k, flags, bad[:5], got[bad[:3]], {kk: want[kk][bad[:3]] for kk in want})
    L = np.linalg.norm(geo.u(seg[:, 4:7]).astype(np.float64) - geo.u(seg[:, 0:3]).astype(np.float64), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = 1e-5 + np.where(L > 0, 2e-3 / L, 0)
    dt = np.abs(got["t"].astype(np.float64) - want["t"])
    assert not (ok & (dt > tol)).any()
    return want, ok


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_segments(name):
    cfg, g, geo, vox, ot = scene(name)
    size = np.float32(cfg["voxel_size"])
    table, _, _ = case_motions("swept_cloud", cfg, geo.N)
    mo = fc.motions([t for t, _ in table], [w for _, w in table])
    g.forecast_update(mo, HORIZONS, True)
    ref = fc.Field(geo, vox, cfg["voxel_size"], mo, HORIZONS, True, occ_track=ot)
    assert fc.equal_fields(*g.forecast()[:3], ref) is None
    seg = random_segments(geo, size)
    states = set()
    for flags in (dict(), dict(unknown_blocks=True), dict(vacated_blocks=True), dict(unknown_blocks=True, vacated_blocks=True)):
        got = g.query_forecast_segments(seg, **flags)
        want, ok = check_segments(geo, ref, seg, got, flags)
        print(name, flags, "excluded %.2f %%" % (100 * (1 - ok.mean())), "hits", int((got["t"] >= 0).sum()))
        assert 1 - ok.mean() <= SEG_EXCLUDED_MAX
        states |= set(got["state"][ok & (got["t"] >= 0)].tolist())
        hand = hand_segments(geo, size)
        hgot = g.query_forecast_segments(hand, **flags)
        hwant, hok = check_segments(geo, ref, hand, hgot, flags)
        assert hok[:4].all()
        ub = bool(flags.get("unknown_blocks"))
        assert (hgot["cells"][4:] == 0).all() and (hgot["t"][4:] == (0.0 if ub else -1.0)).all() and (hgot["cell"][4:] == fc.NOTHING).all()
        assert hgot["cells"][0] == 1 and hgot["cells"][1] == 0 and hgot["t"][1] == (0.0 if ub else -1.0)
        assert (hgot["cells"][2] == 0 and hgot["t"][2] == 0.0) if ub else (hgot["cells"][2] >= 1 and hgot["t"][2] != 0.0)
    if name != "A":
        assert states >= {1, 2, 3, -1}, states
    # no motions, no flags: t, cells and the hit cell are the segment query's, bit for bit
    g.forecast_update(None, HORIZONS)
    plain = g.query_segments(seg[:, 0:3], seg[:, 4:7])
    got = g.query_forecast_segments(seg)
    assert got["t"].tobytes() == plain["t"].tobytes() and np.array_equal(got["cells"], plain["cells"])
    hit = got["cell"] != fc.NOTHING
    assert np.array_equal(hit, plain["voxel"] != qr.INVALID) and hit.any()
    c = got["cell"][hit].astype(np.int64)
    cells = np.stack([c % geo.N[0], (c // geo.N[0]) % geo.N[1], c // (geo.N[0] * geo.N[1])], 1)
    assert np.array_equal(geo.voxel(cells), plain["voxel"][hit]) and (got["state"][hit] == 1).all()


def face_segments(geo, size):
    """axis-parallel segments that lie in the plane of a cell face: inside the map, along its min face, and leaving it"""
    lo, N = geo.center + geo.pmin, geo.N
    rows = []
    for ax in range(3):
        for along in ((ax + 1) % 3, (ax + 2) % 3):
            for plane in (0, 1, int(N[ax]) // 2, int(N[ax]) - 1, int(N[ax])):
                a = (N // 2).astype(np.float32) + np.array([0.5, 0.25, 0.75], np.float32)
                a[ax] = plane
                for start, end in ((0.5, N[along] - 0.5), (N[along] - 1.5, -3.0), (-2.0, N[along] + 2.0)):
                    p, q = a.copy(), a.copy()
                    p[along], q[along] = start, end
                    rows.append(list(lo + p * size) + [0.0] + list(lo + q * size) + [0.0])
    return np.array(rows, np.float32)


@pytest.mark.parametrize("name", ["A", "B", "driven-T0"])
def test_a_forecast_without_motions_walks_like_the_segment_query(name):
    """k_query_forecast_segments and k_query_segments share one walk (sdm_walk.h): with no motions and ta = tb = 0 the two
    answer alike on every segment, ambiguous ones included - t and cells byte for byte, the hit cell through the ring."""
    if name in sc.ALL_CASES:
        cfg, g, geo, vox, _ = scene(name)
    else:
        cfg, g, geo, vox = get_map(*name.split("-"))
    size = np.float32(cfg["voxel_size"])
    seg = np.concatenate([random_segments(geo, size, n=3000, seed=11), hand_segments(geo, size), face_segments(geo, size)])
    seg[:, 3] = seg[:, 7] = 0.0
    a, b = seg[:, 0:3], seg[:, 4:7]
    inside = lambda p: ((geo.u(p) >= 0) & (geo.u(p) < geo.N)).all(axis=1)
    assert (~inside(a)).sum() > 100 and (a == b).all(axis=1).any() and not np.isfinite(seg).all()
    g.forecast_update(None, HORIZONS)
    for ub in (False, True):
        plain = g.query_segments(a, b, unknown_blocks=ub)
        got = g.query_forecast_segments(seg, unknown_blocks=ub)
        print(name, "unknown_blocks", ub, "hits", int((plain["t"] >= 0).sum()), "misses", int((plain["cells"] == 0).sum()))
        assert got["t"].tobytes() == plain["t"].tobytes() and got["cells"].tobytes() == plain["cells"].tobytes()
        hit = got["cell"] != fc.NOTHING
        assert np.array_equal(hit, plain["voxel"] != qr.INVALID) and hit.any() and (plain["cells"] == 0).any()
        c = got["cell"][hit].astype(np.int64)
        cells = np.stack([c % geo.N[0], (c // geo.N[0]) % geo.N[1], c // (geo.N[0] * geo.N[1])], 1)
        assert np.array_equal(geo.voxel(cells), plain["voxel"][hit])
        occupied = (plain["voxel"] != qr.INVALID) & (plain["occ"] >= 1)
        assert occupied.any() and (got["state"][occupied] == 1).all()
        assert ((got["state"][hit & ~occupied] == -1) & (plain["occ"][hit & ~occupied] == -1)).all() and (ub or not (hit & ~occupied).any())


# ---- the rules --------------------------------------------------------------------------------------------------------------
def _moving_tracks(g, vox, cfg):
    t = np.unique(vox["track"][(vox["occ"] >= 1) & (vox["track"] >= 1) & (vox["track"] <= cfg["max_movable_track"])])
    return t[:16]


def test_snapshot_and_stream_order():
    """Build after frame k, then two more frames (ring shifts), a clear and a load_state, nothing synchronised in between:
    field, cell list and queries are frame k's.  A new build gives the new frame's."""
    cfg, params, frames = synth.make_frames("T0", 8, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames[:4]:
        g.update(*f)
    g.synchronize()
    geo_k, vox_k = qr.Geometry(cfg, g.ring_state()), g.voxels()
    state_k = g.dump_state()
    tracks = _moving_tracks(g, vox_k, cfg)
    assert len(tracks) >= 1
    mo = fc.motions(tracks, np.random.default_rng(4).normal(0, 1.0, (len(tracks), 3)))
    g.forecast_update(mo, HORIZONS, True)
    for f in frames[4:6]:
        g.update(*f)
    g.clear()
    g.load_state(state_k)
    mask, first, info, origin = g.forecast()
    ref = fc.Field(geo_k, vox_k, cfg["voxel_size"], mo, HORIZONS, True)
    assert fc.equal_fields(mask, first, info, ref) is None and info["n_marked"] > 0
    assert np.array_equal(origin, (geo_k.center + geo_k.pmin).astype(np.float32))
    assert np.array_equal(g.forecast_cells()[0], ref.cells()[0])
    pts = sample_points(geo_k, np.float32(cfg["voxel_size"]), ref, 4096, 2)
    assert fc.equal_records(g.query_forecast(pts), ref.query(pts), ("state", "horizon", "track", "mask", "first_horizon")) is None   # (frame k's geometry)
    g.clear()
    for f in frames[:7]:
        g.update(*f)
    g.synchronize()
    geo_n, vox_n = qr.Geometry(cfg, g.ring_state()), g.voxels()
    assert not np.array_equal(geo_k.eq, geo_n.eq) or not np.array_equal(geo_k.center, geo_n.center)
    mask_n, _, _, new = check_build(cfg, g, geo_n, vox_n, mo, HORIZONS, True)
    assert not np.array_equal(new.mask, ref.mask)
    g.close()


def test_forecast_leaves_the_map_alone():
    cfg, params, frames = synth.make_frames("T0", 6, n_dynamic=2)
    a = binding.SdmMap(cfg, params, synth.noise_table())
    b = binding.SdmMap(cfg, params, synth.noise_table())
    pts = np.random.default_rng(1).uniform(-3, 3, (512, 4)).astype(np.float32)
    seg = np.random.default_rng(2).uniform(-3, 3, (512, 8)).astype(np.float32)
    seg[:, 7] = np.abs(seg[:, 3]) + 1
    seg[:, 3] = np.abs(seg[:, 3])
    mo = fc.motions(np.arange(1, 33), np.random.default_rng(3).normal(0, 1.0, (32, 3)))
    for i, f in enumerate(frames):
        a.update(*f)
        b.update(*f)
        b.forecast_update(mo, HORIZONS, swept=bool(i & 1))
        b.query_forecast(pts)
        b.query_forecast_segments(seg, unknown_blocks=bool(i & 2))
        b.forecast_cells()
    a.synchronize()
    b.synchronize()
    rep = pu.compare_maps(a, b, a.S, check_results=True)
    assert not rep, "\n".join(rep)
    assert np.array_equal(a.voxels().view(np.uint64), b.voxels().view(np.uint64))
    sa, sb = a.dump_state(), b.dump_state()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    start = np.arange(0, a.V, 97, dtype=np.uint32)
    for m in (a, b):
        m.esdf_update()
        m.frontiers_update()
        m.instances_update()
        m.reach_update(start_cells=start, through_unknown=True)
    for x, y in zip(a.esdf()[:2], b.esdf()[:2]):
        assert np.array_equal(x, y)
    assert a.frontiers()[0].tobytes() == b.frontiers()[0].tobytes()
    assert a.instances()[0].tobytes() == b.instances()[0].tobytes()
    assert np.array_equal(a.reach()[0], b.reach()[0])
    views = np.zeros(4, binding.VIEW)
    views["q"][:, 0], views["range"] = 1.0, 3.0
    dirs = binding.pinhole_rays(cfg, stride=8)
    assert a.query_views(views, dirs).tobytes() == b.query_views(views, dirs).tobytes()
    a.close()
    b.close()


def test_run_to_run_and_modes():
    """five builds: the same bytes; queries on the host and on the device: the same bytes"""
    cfg, g, geo, vox = get_map("dense", "T0")
    tracks = _moving_tracks(g, vox, cfg)
    assert len(tracks) >= 3
    mo = fc.motions(tracks, np.random.default_rng(6).normal(0, 1.2, (len(tracks), 3)))
    ref = fc.Field(geo, vox, cfg["voxel_size"], mo, HORIZONS, True)
    pts = sample_points(geo, np.float32(cfg["voxel_size"]), ref, 4096, 5)
    seg = random_segments(geo, np.float32(cfg["voxel_size"]))
    runs = []
    for _ in range(5):
        g.forecast_update(mo, HORIZONS, True)
        mask, first, info, _ = g.forecast()
        cells = g.forecast_cells()
        runs.append((mask.tobytes(), first.tobytes(), info.tobytes(), b"".join(x.tobytes() for x in cells), g.query_forecast(pts).tobytes(),
                     g.query_forecast_segments(seg, unknown_blocks=True).tobytes()))
    assert all(r == runs[0] for r in runs[1:])
    assert fc.equal_fields(mask, first, info, ref) is None and info["n_marked"] > 0
    d_pts, d_seg = g.device_put(pts), g.device_put(seg)
    d_res, d_hit = g.device_alloc(4096 * 8), g.device_alloc(len(seg) * 16)
    g.forecast_update(mo, HORIZONS, True)   # (in between: the queries read the new build)
    g.query_forecast(d_pts, on_device=True, n=4096, out=d_res)
    g.query_forecast_segments(d_seg, unknown_blocks=True, on_device=True, n=len(seg), out=d_hit)
    g.synchronize()
    assert g.device_download(d_res, 4096 * 8, binding.FORECAST_RESULT).tobytes() == runs[0][4]
    assert g.device_download(d_hit, len(seg) * 16, binding.FORECAST_HIT).tobytes() == runs[0][5]
    for p in (d_pts, d_seg, d_res, d_hit):
        g.device_free(p)


def test_argument_errors():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    L, INV = g.L, 1
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    mo, t = fc.motions([3, 5], np.ones((2, 3))), np.array([0.5, 1.0], np.float32)
    pts, seg = np.zeros((4, 4), np.float32), np.zeros((4, 8), np.float32)
    res, hit = np.zeros(4, binding.FORECAST_RESULT), np.zeros(4, binding.FORECAST_HIT)
    info, n = np.zeros(1, binding.FORECAST_INFO), C.c_int64(0)
    # before any build
    assert L.sdm_get_forecast(g.h, None, None, vp(info), None) == INV and "sdm_forecast_update" in L.sdm_last_error().decode()
    assert L.sdm_get_forecast_cells(g.h, None, None, None, 0, C.byref(n)) == INV
    assert L.sdm_query_forecast(g.h, vp(pts), 4, vp(res), 0) == INV and "sdm_forecast_update" in L.sdm_last_error().decode()
    assert L.sdm_query_forecast_segments(g.h, vp(seg), 4, vp(hit), 0) == INV
    for call in (g.forecast, g.forecast_cells, lambda: g.query_forecast(pts), lambda: g.query_forecast_segments(seg)):
        with pytest.raises(binding.SdmError):
            call()
    # the build's arguments (the rest: tests/test_forecast_abi.py, on the routine the build shares with sdm_forecast_stamps)
    above = fc.motions([cfg["max_movable_track"] + 1], np.ones((1, 3)))
    assert L.sdm_forecast_update(g.h, vp(above), 1, vp(t), 2, 0) == INV and "max_movable_track" in L.sdm_last_error().decode()
    assert L.sdm_forecast_update(g.h, vp(fc.motions([3, 3], np.ones((2, 3)))), 2, vp(t), 2, 0) == INV
    assert L.sdm_forecast_update(g.h, vp(mo), 2, vp(t[::-1].copy()), 2, 0) == INV
    assert L.sdm_forecast_update(g.h, vp(mo), 2, vp(t), 2, 0x2) == INV
    assert L.sdm_forecast_update(g.h, vp(mo), 2, vp(t), 0, 0) == INV
    many = fc.motions(np.arange(1, 4098), np.zeros((4097, 3)))
    assert L.sdm_forecast_update(g.h, vp(many), 4097, vp(np.arange(1, 17, dtype=np.float32)), 16, 0) == 4   # 65552 stamps: SDM_ERR_CAPACITY
    assert L.sdm_get_forecast(g.h, None, None, None, None) == INV                                             # ... and nothing was built
    assert L.sdm_forecast_update(g.h, None, 0, vp(t), 2, 0) == 0
    assert L.sdm_forecast_update(g.h, vp(mo), 2, vp(t), 2, 1) == 0
    assert L.sdm_get_forecast(g.h, None, None, None, None) == 0 and L.sdm_get_forecast(g.h, None, None, vp(info), None) == 0
    assert info[0]["flags"] == 1 and info[0]["n_motions"] == 2 and info[0]["n_sources"] == 0 and info[0]["n_marked"] == 0   # a fresh map
    assert L.sdm_get_forecast_cells(g.h, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert L.sdm_get_forecast_cells(g.h, None, None, None, -1, C.byref(n)) == INV and L.sdm_get_forecast_cells(g.h, None, None, None, 0, None) == INV
    # the queries' arguments; n == 0 launches nothing
    assert L.sdm_query_forecast(g.h, None, 4, vp(res), 0) == INV and L.sdm_query_forecast(g.h, vp(pts), 4, None, 0) == INV
    assert L.sdm_query_forecast(g.h, vp(pts), -1, vp(res), 0) == INV and L.sdm_query_forecast(g.h, vp(pts), 4, vp(res), 0x2) == INV
    assert L.sdm_query_forecast(g.h, vp(pts), 0, vp(res), 0) == 0
    now = -1 if g.voxels()["occ"][0] == -1 else 0   # (a map without a frame reads the same everywhere)
    assert L.sdm_query_forecast(g.h, vp(pts), 4, vp(res), 0) == 0 and (res["state"] == now).all() and (res["horizon"] == 0).all()
    assert (res["first_horizon"] == 0xFF).all() and (res["mask"] == 0).all()
    assert L.sdm_query_forecast_segments(g.h, None, 4, vp(hit), 0) == INV and L.sdm_query_forecast_segments(g.h, vp(seg), 4, None, 0) == INV
    assert L.sdm_query_forecast_segments(g.h, vp(seg), 4, vp(hit), 0x8) == INV
    assert L.sdm_query_forecast_segments(g.h, vp(seg), 0, vp(hit), 0) == 0
    assert L.sdm_query_forecast_segments(g.h, vp(seg), 4, vp(hit), 0x6) == 0 and (hit["cells"] == 1).all()
    assert (hit["state"] == now).all() and (hit["t"] == (0 if now == -1 else -1)).all()
    g.close()
    s = binding.SdmMap(cfg, PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert s.L.sdm_forecast_update(s.h, vp(mo), 2, vp(t), 2, 0) == INV and "shard" in s.L.sdm_last_error().decode()
    assert s.L.sdm_get_forecast(s.h, None, None, vp(info), None) == INV
    assert s.L.sdm_get_forecast_cells(s.h, None, None, None, 0, C.byref(n)) == INV
    assert s.L.sdm_query_forecast(s.h, vp(pts), 4, vp(res), 0) == INV
    assert s.L.sdm_query_forecast_segments(s.h, vp(seg), 4, vp(hit), 0) == INV
    with pytest.raises(binding.SdmError):
        s.forecast_update(mo, t)
    s.close()
