"""The ground layer (include/sdm.h: sdm_ground_update / sdm_get_ground / sdm_query_ground / sdm_query_footprints) against
tests/ground_ref.py, bit for bit: cells, d2, the info block, the origin, the query results (floats by their bit patterns).

Crafted maps on every shape of tests/shape_cases.py, the ring shifted on every axis, under all six orientations; the
filled maps of tests/test_instances_gpu.py; the queries in host and device mode; the snapshot rule; no side effects;
run-to-run identity; the argument checks."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import esdf_ref as er
from tests import ground_ref as gr
from tests import parity_utils as pu
from tests import query_ref as qr
from tests import shape_cases as sc
from tests.test_instances_gpu import DRIVE, MAPS, get_map

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
ROAD, BUILDING, CAR = synth.LABEL_ROAD, synth.LABEL_BUILDING, synth.LABEL_CAR
ORIENTATIONS = [(a, s) for a in (0, 1, 2) for s in (1, -1)]
# cell kinds of a crafted column: (occ, label, track)
FLOOR = (1, ROAD, synth.TRACK_ROAD)
BOX = (1, BUILDING, synth.TRACK_BUILDING)          # solid, but its label carries nobody (unless the mask says so)
ROOF = (1, CAR, 3)                                 # a movable object's cell
RIDER = (1, ROAD, 5)                               # a movable track under a supporting label: never a support
UNKNOWN = (-1, 0, 0)


def _dims(cfg):
    return np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.int64)


def column_types(N):
    """crafted columns as {height: kind}, heights for up_sign +1; every type also mirrored (h -> N - 1 - h), so that both
    signs meet every feature; types that do not fit N cells are left out"""
    t = [
        {},                                          # nothing: class 0
        {0: FLOOR},
        {1: FLOOR},
        {2: FLOOR},
        {3: FLOOR},
        {0: FLOOR, 1: BOX},                          # a box on the floor
        {0: FLOOR, 3: FLOOR},                        # a table: floor, a gap of two, a slab
        {0: FLOOR, 2: ROOF},                         # a movable roof one cell above the floor
        {0: RIDER},
        {1: FLOOR, 2: UNKNOWN},                      # unknown cells in the headroom
        {0: FLOOR, 1: UNKNOWN, 2: UNKNOWN, 3: BOX},
        {h: UNKNOWN for h in range(N)},
        {N - 1: FLOOR},                              # the clearance runs out of the map's top
        {N - 2: FLOOR},
        {0: BOX, N - 1: BOX},
    ]
    for h in (62, 63, 64):                           # a support whose clearance cells straddle a 64-cell chunk boundary
        t += [{h: FLOOR, h + 3: BOX}, {h: FLOOR, h + 2: UNKNOWN}, {h - 2: FLOOR, h: FLOOR, h + 1: ROOF}]
    t += [{N // 2: FLOOR, N // 2 + 5: FLOOR, N // 2 + 300: BOX}]   # headroom above 255
    t = [c for c in t if all(0 <= h < N for h in c)]
    return t + [{N - 1 - h: k for h, k in c.items()} for c in t]


def crafted_block(cfg, up_axis, seed=0):
    """-> (occ, label, track) [z, y, x]: the column types dealt over the grid so that neighbours differ (steps of every
    size, on the grid's edges and across the ring's wrap point alike)"""
    N = _dims(cfg)
    au, av = gr.grid_axes(up_axis)
    types = column_types(int(N[up_axis]))
    occ, label, track = (np.zeros(tuple(N[::-1]), dt) for dt in (np.int8, np.uint8, np.uint16))
    rng = np.random.default_rng(1000 + seed)
    pick = rng.integers(0, len(types), (int(N[av]), int(N[au])))
    for j in range(int(N[av])):
        for i in range(int(N[au])):
            for h, (o, l, t) in types[pick[j, i]].items():
                idx = [0, 0, 0]
                idx[up_axis], idx[au], idx[av] = h, i, j
                occ[idx[2], idx[1], idx[0]], label[idx[2], idx[1], idx[0]], track[idx[2], idx[1], idx[0]] = o, l, t
    return occ, label, track


def random_block(cfg, seed):
    N = _dims(cfg)
    rng = np.random.default_rng(seed)
    shape = tuple(N[::-1])
    occ = rng.choice(np.array([-1, 0, 0, 0, 1], np.int8), size=shape)
    label = rng.choice(np.array([ROAD, ROAD, BUILDING, CAR], np.uint8), size=shape)
    track = rng.choice(np.array([synth.TRACK_ROAD, synth.TRACK_BUILDING, 3, 5], np.uint16), size=shape)
    return occ, label, track


def _cells(mask):
    z, y, x = np.nonzero(mask)
    return np.stack([x, y, z], axis=1)


def crafted_map(cfg, occ, label, track):
    """a map on a ring shifted on every axis whose result array reads the block: the state is loaded, one frame that sees
    nothing writes every result (as tests/test_frontiers_gpu.py::crafted_map does, with labels and tracks)"""
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    solid = _cells(occ == 1)
    g.load_state(sc.crafted_state(cfg, ring, solid, _cells(occ == -1), tracks=track[occ == 1], labels=label[occ == 1]))
    g.set_ring_state(ring)
    depth = np.full((cfg["height"], cfg["width"]), np.nan, np.float32)
    cloud = np.zeros(cfg["height"] * cfg["width"], synth.LABELED_POINT)
    g.update(depth, cloud, np.array(ring["last_pos"], np.float32), synth.yaw_quat(0.0).astype(np.float32), None, sync=True)
    geo, vox = qr.Geometry(cfg, g.ring_state()), g.voxels()
    assert all(e != 0 for e in geo.eq)
    snap = er.snapshot_grid(geo, vox)
    got_occ = ((snap >> 24) & 0xFF).astype(np.uint8).view(np.int8)
    assert np.array_equal(np.minimum(got_occ, 1), occ)                     # (an obstacle reads 1 or 2)
    assert np.array_equal(((snap >> 16) & 0xFF)[occ == 1], label[occ == 1]) and np.array_equal((snap & 0xFFFF)[occ == 1], track[occ == 1])
    return g, geo, snap


def check_build(cfg, g, geo, snap, opt):
    """one build against the restatement -> (cells, d2, info) of the reference"""
    g.ground_update(**gr.update_kwargs(opt))
    cells, d2, info, origin = g.ground()
    want_cells, want_d2, want_info = gr.build(snap, cfg["max_movable_track"], opt)
    for name in binding.GROUND_CELL.names:
        bad = np.argwhere(cells[name] != want_cells[name])
        assert not len(bad), (opt, name, len(bad), bad[:4].tolist(), cells[tuple(bad[0])], want_cells[tuple(bad[0])])
    assert cells.tobytes() == want_cells.tobytes()
    bad = np.argwhere(d2 != want_d2)
    assert not len(bad), (opt, "d2", len(bad), bad[:4].tolist())
    msg = gr.check_info(info, want_info, opt)
    assert msg is None, (opt, msg)
    assert origin.tobytes() == gr.origin_of(geo).tobytes()
    return want_cells, want_d2, want_info


def option_sets(up, N):
    full = (0, N - 1)
    return [
        gr.options(up, *full, clearance=2, max_step=1, labels=[ROAD]),
        gr.options(up, 1, N - 2, clearance=1, max_step=0, labels=[ROAD], flags=gr.IGNORE_MOVABLE | gr.UNKNOWN_PASSABLE),
        gr.options(up, *full, clearance=3, max_step=2, labels=[ROAD, BUILDING], flags=gr.NONE_IS_LETHAL),
        gr.options(up, *full, clearance=0, max_step=65535, labels=[]),                           # an empty label mask
        gr.options(up, *full, clearance=255, max_step=1, labels=[ROAD], flags=gr.UNKNOWN_PASSABLE),
        gr.options(up, *full, clearance=2, max_step=1, labels=[ROAD], flags=gr.IGNORE_MOVABLE),
        gr.options(up, N // 2, N // 2, clearance=1, max_step=3, labels=[ROAD, CAR], flags=gr.UNKNOWN_PASSABLE | gr.NONE_IS_LETHAL),
    ]


# ---- crafted maps: every shape, every up axis, both signs ----------------------------------------------------------------
@pytest.mark.parametrize("up_axis", [0, 1, 2])
@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_crafted_maps(name, up_axis):
    cfg = sc.config(name)
    N = int(_dims(cfg)[up_axis])
    g, geo, snap = crafted_map(cfg, *crafted_block(cfg, up_axis, seed=ord(name) + up_axis))
    au, av = gr.grid_axes(up_axis)
    big = int(geo.N[au] * geo.N[av]) > 65536       # (the restatement's distance transform is the slow part there)
    seen = dict(step=0, edge_step=0, ground=0, obstacle=0, none=0)
    for sign in (1, -1):
        sets = option_sets((up_axis, sign), N)
        for opt in (sets[:2] if big else sets):
            cells, d2, info = check_build(cfg, g, geo, snap, opt)
            step = (cells["cls"] & 4) != 0
            seen["step"] += int(step.sum())
            seen["edge_step"] += int(step[0].sum() + step[-1].sum() + step[:, 0].sum() + step[:, -1].sum())
            seen["ground"], seen["obstacle"], seen["none"] = (seen[k] + info["n_" + k] for k in ("ground", "obstacle", "none"))
            if opt["labels"] == []:
                assert info["n_ground"] == 0 and info["n_step"] == 0
    assert all(v > 0 for v in seen.values()), seen
    g.close()


def test_kerbs_at_the_edge_and_across_the_wrap_point():
    """a flat floor with one-cell-wide kerbs of max_step and of max_step + 1 cells: on the grid's edge and on both sides of
    the ring's wrap point, on every up axis"""
    cfg = sc.config("F")
    N = _dims(cfg)
    for up_axis in (0, 1, 2):
        au, av = gr.grid_axes(up_axis)
        ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
        wrap = (N - qr.Geometry(cfg, ring).eq) % N                 # the map cells whose ring index is 0
        level = np.zeros((int(N[av]), int(N[au])), np.int64)
        rows = [0, int(wrap[av]) - 1, int(wrap[av]), int(N[av]) - 1]
        cols = [0, int(wrap[au]) - 1, int(wrap[au]), int(N[au]) - 1]
        level[rows[0], 5], level[rows[1], 7], level[rows[2], 9], level[rows[3], 11] = 2, 3, 2, 3
        level[5, cols[0]], level[7, cols[1]], level[9, cols[2]], level[11, cols[3]] = 3, 2, 3, 2
        level[int(wrap[av]) - 1, int(wrap[au]) - 1], level[int(wrap[av]), int(wrap[au])] = 2, 5
        occ, label, track = (np.zeros(tuple(N[::-1]), dt) for dt in (np.int8, np.uint8, np.uint16))
        jj, ii = np.nonzero(level >= 0)
        idx = [None, None, None]
        idx[up_axis], idx[au], idx[av] = level[jj, ii], ii, jj
        occ[idx[2], idx[1], idx[0]], label[idx[2], idx[1], idx[0]], track[idx[2], idx[1], idx[0]] = FLOOR
        g, geo, snap = crafted_map(cfg, occ, label, track)
        opt = gr.options((up_axis, 1), 0, int(N[up_axis]) - 1, clearance=2, max_step=2, labels=[ROAD])
        cells, d2, info = check_build(cfg, g, geo, snap, opt)
        step = (cells["cls"] & 4) != 0
        assert np.array_equal(step, level >= 3) and info["n_step"] == 5 and info["n_lethal"] == 5 and info["n_ground"] == level.size
        assert (cells["level"] == level).all() and info["level_min"] == 0 and info["level_max"] == 5
        check_build(cfg, g, geo, snap, gr.options((up_axis, 1), 0, int(N[up_axis]) - 1, clearance=2, max_step=1, labels=[ROAD]))
        g.close()


@pytest.mark.parametrize("name", ["A", "C", "D"])     # (D: rows and columns of 512 with the nearest lethal column far away)
def test_no_lethal_column_and_one_in_a_corner(name):
    cfg = sc.config(name)
    N = _dims(cfg)
    for up_axis in (0, 1, 2):
        au, av = gr.grid_axes(up_axis)
        for corner in (False, True):
            occ, label, track = (np.zeros(tuple(N[::-1]), dt) for dt in (np.int8, np.uint8, np.uint16))
            sl = [slice(None)] * 3
            sl[2 - up_axis] = 0
            occ[tuple(sl)], label[tuple(sl)], track[tuple(sl)] = FLOOR      # a floor on index 0 of the up axis
            if corner:                                                     # a box on it at column (N_u - 1, N_v - 1)
                idx = [0, 0, 0]
                idx[up_axis], idx[au], idx[av] = 1, N[au] - 1, N[av] - 1
                occ[idx[2], idx[1], idx[0]], label[idx[2], idx[1], idx[0]], track[idx[2], idx[1], idx[0]] = BOX
            g, geo, snap = crafted_map(cfg, occ, label, track)
            for sign in (1, -1):                   # sign -1: the floor is the map's top cell, the box hangs below it
                opt = gr.options((up_axis, sign), 0, int(N[up_axis]) - 1, clearance=1, max_step=0, labels=[ROAD])
                cells, d2, info = check_build(cfg, g, geo, snap, opt)
                if corner and sign > 0:
                    assert info["n_lethal"] == 1 and d2[-1, -1] == 0 and d2[0, 0] == (N[au] - 1) ** 2 + (N[av] - 1) ** 2
                else:
                    assert info["n_lethal"] == 0 and (d2 == gr.INVALID).all() and info["n_ground"] == d2.size
                pts = gr.origin_of(geo) + (np.array([[0.5, 0.5, 0.5], [1.5, 2.5, 3.5]]) * cfg["voxel_size"]).astype(np.float32)
                got = g.query_ground(pts)
                assert got.tobytes() == gr.query_ground(geo, cfg["voxel_size"], opt, cells, d2, pts).tobytes()
                assert (got["dist"] == -1).all() == (info["n_lethal"] == 0)
            g.close()


def test_random_block_of_32_cells_per_axis():
    cfg = dict(synth.CONFIGS["T0"])
    g, geo, snap = crafted_map(cfg, *random_block(cfg, 9))
    for up in ORIENTATIONS:
        for opt in option_sets(up, 32)[:5]:
            check_build(cfg, g, geo, snap, opt)
    g.close()


# ---- filled maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", MAPS)
def test_filled_maps(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    snap = er.snapshot_grid(geo, vox)
    labels = sorted(set(np.unique((snap >> 16) & 0xFF).tolist()[::2]) | {ROAD})
    for up in ((1, -1), (2, 1)):
        N = int(geo.N[up[0]])
        for k, opt in enumerate((gr.options(up, 0, N - 1, 2, 1, labels), gr.options(up, N // 4, N - 2, 1, 0, labels, gr.IGNORE_MOVABLE),
                                 gr.options(up, 2, N // 2, 3, 2, labels, gr.UNKNOWN_PASSABLE | gr.NONE_IS_LETHAL))):
            cells, d2, info = check_build(cfg, g, geo, snap, opt)
            if kind == "dense" and k == 2:
                assert info["n_ground"] > 0 and info["n_lethal"] > 0


# ---- the queries -------------------------------------------------------------------------------------------------------------
def query_points(geo, size, rng, n):
    N = geo.N
    lo = (geo.center + geo.pmin).astype(np.float64)
    hi = lo + N * float(size)
    pts = rng.uniform(lo - 2 * size, hi + 2 * size, (n, 3))
    pts[: n // 2] = rng.uniform(lo, hi, (n // 2, 3))
    k = 0
    for a in range(3):                             # the map's faces, and the u in (-1, 0) sliver below each
        for v in (lo[a], hi[a], lo[a] - 0.5 * size, np.nextafter(np.float32(hi[a]), np.float32(-np.inf)), lo[a] + 1e-4):
            pts[k] = rng.uniform(lo, hi)
            pts[k, a] = v
            k += 1
    pts[k:k + 4] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]]
    return pts.astype(np.float32)


def footprints(geo, size, up_axis, rng, n):
    au, av = gr.grid_axes(up_axis)
    o = gr.origin_of(geo).astype(np.float64)
    span = np.array([geo.N[au], geo.N[av]]) * float(size)
    fps = np.zeros(n, binding.FOOTPRINT)
    th = rng.uniform(0, 2 * np.pi, n)
    fps["center_u"], fps["center_v"] = o[au] + rng.uniform(-0.1, 1.1, n) * span[0], o[av] + rng.uniform(-0.1, 1.1, n) * span[1]
    fps["dir_u"], fps["dir_v"] = np.cos(th), np.sin(th)
    fps["half_len"], fps["half_wid"] = rng.uniform(0.3, 9.0, n) * size, rng.uniform(0.2, 5.0, n) * size
    for k, d in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):        # axis-aligned: whole columns, edges on column borders
        fps[k] = (o[au] + 6 * size, o[av] + 5 * size, d[0], d[1], 3 * size, 2 * size)
    fps[4] = (o[au], o[av] + 0.5 * span[1], 1, 0, 4 * size, 2.5 * size)               # on the grid's edge: half of it outside
    fps[5] = (o[au] + span[0], o[av] + span[1], 0.6, 0.8, 5 * size, 3 * size)         # on the far corner
    fps[6] = (o[au] + 0.5 * span[0], o[av] + 0.5 * span[1], 1, 0, 40 * size, 24.5 * size)   # too large
    fps[7] = (o[au] + 0.5 * span[0], o[av] + 0.5 * span[1], 1, 0, 40 * size, 24 * size)     # the largest allowed
    fps[8] = fps[9] = fps[10] = fps[11] = fps[0]
    fps[8]["center_v"], fps[9]["dir_u"], fps[10]["half_len"], fps[11]["half_wid"] = np.nan, np.inf, -np.inf, np.nan
    fps[12] = (o[au] + 3 * size, o[av] + 3 * size, 1, 0, 0.2 * size, 0.2 * size)      # on a corner of four columns: covers none
    o32, f32 = gr.origin_of(geo), np.float32
    fps[13] = (o32[au] + f32(3.5) * f32(size), o32[av] + f32(3.5) * f32(size), 1, 0, 0, 0)   # a column's centre alone, as the rule forms it
    fps[14] = (o[au] + 0.5 * span[0], o[av] + 0.5 * span[1], 0, 0, 1 * size, 1 * size)  # no heading: every column passes the rule
    fps[15] = (o[au] + 0.5 * span[0], o[av] + 0.5 * span[1], 0.5, 0.5, 6 * size, 1 * size)  # a heading of length 0.7
    fps[16] = (1e30, -1e30, 1, 0, 2 * size, 1 * size)                                 # finite, far away
    fps[17] = (o[au] + 10 * size, o[av] + 10 * size, 0.8, -0.6, -1 * size, 2 * size)  # a negative half length covers nothing
    return fps


@pytest.mark.parametrize("up", ORIENTATIONS)
def test_queries_host_and_device(up):
    cfg = sc.config("F")
    size = cfg["voxel_size"]
    g, geo, snap = crafted_map(cfg, *crafted_block(cfg, up[0], seed=77))
    opt = gr.options(up, 0, int(geo.N[up[0]]) - 1, clearance=2, max_step=1, labels=[ROAD])
    cells, d2, info = check_build(cfg, g, geo, snap, opt)
    assert info["n_lethal"] > 0 and info["n_ground"] > 0
    rng = np.random.default_rng(31 + 7 * up[0] + up[1])
    pts = query_points(geo, size, rng, 600)
    want = gr.query_ground(geo, size, opt, cells, d2, pts)
    assert (want["status"] == 3).sum() >= 10 and (want["above"][want["status"] == 0] > 0).any()
    assert ((want["above"] < 0) & (want["above"] != gr.INT32_MIN)).any() and (want["above"] == gr.INT32_MIN).any()
    host = g.query_ground(pts)
    bad = np.flatnonzero(host != want)
    assert not len(bad), (len(bad), pts[bad[:3]], host[bad[:3]], want[bad[:3]])
    assert host.tobytes() == want.tobytes()
    fps = footprints(geo, size, up[0], rng, 96)
    want_fp = gr.query_footprints(geo, size, opt, cells, d2, fps)
    none = (0, 0, 0, 0, gr.NO_LEVEL, gr.NO_LEVEL, gr.INVALID, gr.INVALID, 0)
    assert all(tuple(int(v) for v in want_fp[k]) == none for k in (6, 8, 9, 10, 11, 12, 16, 17))
    assert want_fp["n_cols"][7] > 0 and want_fp["n_cols"][13] == 1 and want_fp["n_cols"][14] == d2.size and want_fp["n_cols"][0] == 6 * 4
    assert (want_fp["n_lethal"] > 0).any() and (want_fp["n_lethal"] == 0).any()
    host_fp = g.query_footprints(fps)
    bad = np.flatnonzero(host_fp != want_fp)
    assert not len(bad), (bad[:6].tolist(), host_fp[bad[:3]], want_fp[bad[:3]])
    assert host_fp.tobytes() == want_fp.tobytes()
    # device mode: the same bytes
    d_pts, d_out = g.device_put(pts), g.device_alloc(len(pts) * 32)
    d_fps, d_res = g.device_put(fps), g.device_alloc(len(fps) * 32)
    g.query_ground(d_pts, on_device=True, n=len(pts), out=d_out)
    g.query_footprints(d_fps, on_device=True, n=len(fps), out=d_res)
    g.synchronize()
    assert g.device_download(d_out, len(pts) * 32, binding.GROUND_RESULT).tobytes() == want.tobytes()
    assert g.device_download(d_res, len(fps) * 32, binding.FOOTPRINT_RESULT).tobytes() == want_fp.tobytes()
    for p in (d_pts, d_out, d_fps, d_res):
        g.device_free(p)
    g.close()


def test_a_batch_longer_than_one_staging_chunk():
    cfg, g, geo, vox = get_map("driven", "T0")
    snap = er.snapshot_grid(geo, vox)
    opt = gr.options((1, -1), 0, 31, clearance=2, max_step=1, labels=sorted(set(np.unique((snap >> 16) & 0xFF).tolist())))
    cells, d2, info = check_build(cfg, g, geo, snap, opt)
    rng = np.random.default_rng(8)
    n = (1 << 20) + 4099                           # host mode stages 2^20 items at a time
    lo = (geo.center + geo.pmin).astype(np.float64)
    pts = rng.uniform(lo - 0.4, lo + geo.N * float(cfg["voxel_size"]) + 0.4, (n, 3)).astype(np.float32)
    assert g.query_ground(pts).tobytes() == gr.query_ground(geo, cfg["voxel_size"], opt, cells, d2, pts).tobytes()
    fps = footprints(geo, cfg["voxel_size"], 1, rng, 64)
    fps = np.concatenate([fps] * ((n + 63) // 64))[:n]
    got = g.query_footprints(fps)
    want = gr.query_footprints(geo, cfg["voxel_size"], opt, cells, d2, fps[:64])
    assert got[:64].tobytes() == want.tobytes() and got[-64 - n % 64:-(n % 64)].tobytes() == want.tobytes()
    assert got[1 << 20:(1 << 20) + 64].tobytes() == want.tobytes()


# ---- the snapshot rule, side effects, run to run, arguments ---------------------------------------------------------------
def test_snapshot_and_stream_order():
    """Build after frame k, then two more frames (ring shifts) and a clear, nothing synchronised in between: the layer and
    both queries are frame k's.  A new build gives the new frame's."""
    cfg, params, frames = synth.make_frames("T0", 8, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames[:4]:
        g.update(*f)
    g.synchronize()
    geo_k, vox_k = qr.Geometry(cfg, g.ring_state()), g.voxels()
    snap_k = er.snapshot_grid(geo_k, vox_k)
    labels = sorted(set(np.unique((snap_k >> 16) & 0xFF).tolist()))
    opt = gr.options((1, -1), 0, 31, clearance=1, max_step=1, labels=labels)
    g.ground_update(**gr.update_kwargs(opt))
    for f in frames[4:6]:
        g.update(*f)
    g.clear()
    cells, d2, info, origin = g.ground()
    want_cells, want_d2, want_info = gr.build(snap_k, cfg["max_movable_track"], opt)
    assert cells.tobytes() == want_cells.tobytes() and np.array_equal(d2, want_d2) and gr.check_info(info, want_info, opt) is None
    assert origin.tobytes() == gr.origin_of(geo_k).tobytes() and want_info["n_ground"] > 0
    rng = np.random.default_rng(12)
    pts = query_points(geo_k, cfg["voxel_size"], rng, 300)
    assert g.query_ground(pts).tobytes() == gr.query_ground(geo_k, cfg["voxel_size"], opt, cells, d2, pts).tobytes()   # (frame k's geometry)
    fps = footprints(geo_k, cfg["voxel_size"], 1, rng, 32)
    assert g.query_footprints(fps).tobytes() == gr.query_footprints(geo_k, cfg["voxel_size"], opt, cells, d2, fps).tobytes()
    g.update(*frames[6])
    g.synchronize()
    geo_n = qr.Geometry(cfg, g.ring_state())
    new_cells, _, _ = check_build(cfg, g, geo_n, er.snapshot_grid(geo_n, g.voxels()), opt)
    assert new_cells.tobytes() != want_cells.tobytes()
    g.close()


def test_ground_leaves_the_map_alone():
    cfg, params, frames = synth.make_frames("T0", 6, n_dynamic=2)
    a = binding.SdmMap(cfg, params, synth.noise_table())
    b = binding.SdmMap(cfg, params, synth.noise_table())
    rng = np.random.default_rng(3)
    for i, f in enumerate(frames):
        a.update(*f)
        b.update(*f)
        up = ORIENTATIONS[i % 6]
        b.ground_update(up=up, h_lo=0, h_hi=31, clearance=i, max_step=1, support_labels=[ROAD, BUILDING], ignore_movable=bool(i & 1))
        geo = qr.Geometry(cfg, b.ring_state())
        b.query_ground(query_points(geo, cfg["voxel_size"], rng, 200))
        b.query_footprints(footprints(geo, cfg["voxel_size"], up[0], rng, 32))
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
    snap = er.snapshot_grid(geo, vox)
    labels = sorted(set(np.unique((snap >> 16) & 0xFF).tolist()))
    rng = np.random.default_rng(4)
    pts, fps = query_points(geo, cfg["voxel_size"], rng, 400), footprints(geo, cfg["voxel_size"], 0, rng, 48)
    for up in ((0, 1), (2, -1)):
        runs = []
        fps = footprints(geo, cfg["voxel_size"], up[0], rng, 48)
        for _ in range(2):
            g.ground_update(up=up, h_lo=1, h_hi=60, clearance=2, max_step=1, support_labels=labels, unknown_passable=True)
            cells, d2, info, origin = g.ground()
            runs.append((cells.tobytes(), d2.tobytes(), info.tobytes(), origin.tobytes(), g.query_ground(pts).tobytes(),
                         g.query_footprints(fps).tobytes()))
        assert runs[0] == runs[1]
    # other options: nothing of the build before is left
    opt = gr.options((1, 1), 0, 63, 0, 0, labels[:1], gr.NONE_IS_LETHAL)
    cells, d2, info = check_build(cfg, g, geo, snap, opt)
    assert cells.tobytes() != runs[0][0]


def test_argument_errors():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    L, INV = g.L, 1
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pts, out = np.zeros((4, 3), np.float32), np.zeros(4, binding.GROUND_RESULT)
    fps, res = np.zeros(4, binding.FOOTPRINT), np.zeros(4, binding.FOOTPRINT_RESULT)
    info = np.zeros(1, binding.GROUND_INFO)
    # before any build
    assert L.sdm_get_ground(g.h, None, None, vp(info), None) == INV and "sdm_ground_update" in L.sdm_last_error().decode()
    assert L.sdm_query_ground(g.h, vp(pts), 4, vp(out), 0) == INV and "sdm_ground_update" in L.sdm_last_error().decode()
    assert L.sdm_query_footprints(g.h, vp(fps), 4, vp(res), 0) == INV
    for call in (g.ground, lambda: g.query_ground(pts), lambda: g.query_footprints(fps)):
        with pytest.raises(binding.SdmError):
            call()

    def update(**kw):
        o = np.zeros(1, binding.GROUND_OPTIONS)
        o["up_axis"], o["up_sign"], o["h_lo"], o["h_hi"] = 1, -1, 0, 31
        for k, v in kw.items():
            o[k] = v
        return L.sdm_ground_update(g.h, vp(o))

    assert L.sdm_ground_update(g.h, None) == INV
    for bad in (dict(flags=0x8), dict(flags=0x80000000), dict(up_axis=3), dict(up_axis=-1), dict(up_sign=0), dict(up_sign=2),
                dict(h_lo=-1), dict(h_hi=32), dict(h_lo=5, h_hi=4), dict(clearance=256), dict(max_step=65536)):
        assert update(**bad) == INV, bad
        assert L.sdm_get_ground(g.h, None, None, vp(info), None) == INV          # (a refused build is no build)
    for good in (dict(), dict(flags=0x7), dict(h_lo=31), dict(h_hi=0), dict(clearance=255, max_step=65535), dict(up_axis=0, up_sign=1)):
        assert update(**good) == 0, good
    assert L.sdm_get_ground(g.h, None, None, None, None) == 0 and L.sdm_get_ground(g.h, None, None, vp(info), None) == 0
    assert info[0]["n_none"] == 32 * 32 and info[0]["n_lethal"] == 0 and info[0]["level_min"] == gr.NO_LEVEL   # a fresh map: nothing known
    assert info[0]["axis_u"] == 1 and info[0]["axis_v"] == 2 and info[0]["options"]["up_axis"] == 0
    # the queries' arguments
    for fn, a, o in ((L.sdm_query_ground, pts, out), (L.sdm_query_footprints, fps, res)):
        assert fn(g.h, None, 4, vp(o), 0) == INV
        assert fn(g.h, vp(a), 4, None, 0) == INV
        assert fn(g.h, vp(a), -1, vp(o), 0) == INV
        assert fn(g.h, vp(a), 4, vp(o), 0x2) == INV
        assert fn(g.h, vp(a), 0, vp(o), 0) == 0
        assert fn(g.h, vp(a), 4, vp(o), 0) == 0
    g.close()
    s = binding.SdmMap(cfg, PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    o = np.zeros(1, binding.GROUND_OPTIONS)
    o["up_axis"], o["up_sign"], o["h_hi"] = 1, -1, 31
    assert s.L.sdm_ground_update(s.h, vp(o)) == INV and "shard" in s.L.sdm_last_error().decode()
    assert s.L.sdm_get_ground(s.h, None, None, vp(info), None) == INV
    assert s.L.sdm_query_ground(s.h, vp(pts), 4, vp(out), 0) == INV
    assert s.L.sdm_query_footprints(s.h, vp(fps), 4, vp(res), 0) == INV
    with pytest.raises(binding.SdmError):
        s.ground_update(up=(1, -1), h_lo=0, h_hi=31)
    s.close()
