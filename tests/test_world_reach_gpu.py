"""sdm_world_reach_update / sdm_get_world_reach / sdm_query_world_reach / sdm_world_reach_paths (include/sdm.h) against
tests/world_reach_ref.py, bit for bit: coordinates, cost rows, info (without `rounds`), query results and paths.

The archive needs a map only as a handle: every case but the last feeds the hand-written bricks of
tests/world_reach_cases.py to world_import on a fresh map of shape A (4 cells an axis).  The crafted cases (one brick,
rooms, the shell, the late corner, corridor and serpentine, the plate of 2116 bricks, the int16 edge, inflation), the
random archive under every flag combination, budget and box; the snapshot under retain, import and clear; starts; device
mode with canaries; reproducibility and no side effects; frames whose camera leaves what it archived; the argument checks.
The late corner was held to fail without the edge and corner wake-ups on a CPU emulation of the rounds, not
by breaking the build."""
import ctypes as C
import itertools

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import test_world_gpu as twg
from tests import world_reach_cases as wc
from tests import world_reach_ref as wrr
from tests.test_ground_gpu import _cells

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV = 1
CFG, MM = wc.CFG, wc.MM
SIZE = np.float32(CFG["voxel_size"])
NO = wrr.NO_COST
FILL = binding.WORLD_REACH_NO_CELL


def handle():
    return binding.SdmMap(CFG, PARAMS, synth.noise_table())


def world_of(c):
    g = handle()
    g.world_import(c["hdr"], c["cells"])
    hdr, cells = g.world_bricks()
    assert np.array_equal(cells, c["cells"]) and len(hdr) == len(c["hdr"])
    return g


def check_goals(g, ref, goals, size=SIZE, max_len=None):
    """query results and paths for the world cells `goals`, given as cells and as the points of their centres"""
    want = ref.query(size, cells=goals)
    got = g.query_world_reach(cells=goals)
    assert wrr.equal_results(got, want) is None, wrr.equal_results(got, want)
    xyz = wrr.cell_centres(goals, size)
    got_p, want_p = g.query_world_reach(xyz=xyz), ref.query(size, xyz=xyz)
    assert wrr.equal_results(got_p, want_p) is None, wrr.equal_results(got_p, want_p)
    paths = ref.paths(size, cells=goals)
    longest = max([len(p) for p in paths] + [1])
    max_len = longest if max_len is None else max_len
    for kw in (dict(cells=goals), dict(xyz=xyz)):
        rows, lens = g.world_reach_paths(max_len=max_len, **kw)
        assert lens.tolist() == [len(p) for p in paths]
        for row, p in zip(rows, paths):
            k = min(len(p), max_len)
            assert np.array_equal(row[:k], p[:k]) and (row[k:] == FILL).all()
    return want


def check_build(g, c, n_goals=24, seed=7, hdr_cells=None, size=SIZE, **more):
    """one build on the map and in the restatement - fed with the case's bricks, or with what the map itself returns"""
    kw = dict(c["kw"], **more)
    hdr, cells = hdr_cells if hdr_cells is not None else (c["hdr"], c["cells"])
    g.world_reach_update(start_cells=c["starts"], **kw)
    ref = wrr.DenseField(hdr, cells, c["starts"], MM, stamp=int(g.world_info()["stamp"]), **kw)
    got = g.world_reach()
    assert wrr.equal_fields(got, ref) is None, wrr.equal_fields(got, ref)
    if kw.get("box") is None:   # row r of the field is row r of the archive
        b = g.world_bricks(with_cells=False)[0]
        assert np.array_equal(got[0], np.stack([b["bx"], b["by"], b["bz"]], 1))
    check_goals(g, ref, wc.sample_goals(ref, n_goals, seed), size)
    return got, ref


CASES = None


def crafted(name):
    global CASES
    CASES = CASES or wc.crafted()
    return CASES[name]


# ---- 1 - 5, 7, 8 and the inflation: the crafted cases
@pytest.mark.parametrize("name", ["one brick", "one brick at -1", "rooms face", "rooms edge", "rooms corner", "shell through_unknown=False",
                                  "shell through_unknown=True", "late corner", "corridor", "serpentine", "plate face=True", "plate face=False",
                                  "int16 edge", "pillars inflate=1 face=False", "pillars inflate=2 face=False", "pillars inflate=2 face=True",
                                  "ball inflate=1 skip=False", "ball inflate=1 skip=True", "ball inflate=2 skip=False", "ball inflate=2 skip=True"])
def test_crafted_archives(name):
    c = crafted(name)
    g = world_of(c)
    (coords, cost, info), ref = check_build(g, c)
    assert info["n_starts_used"] == len(np.unique(c["starts"], axis=0)) and info["n_reached"] > 0 and info["rounds"] >= 1
    if name.startswith("one brick"):
        for face in (False, True):
            g.world_reach_update(start_cells=c["starts"], face_connected=face)
            want = np.array([wc.closed_form((w & 7, (w >> 3) & 7, w >> 6), face) for w in range(512)], np.uint32)
            assert np.array_equal(g.world_reach()[1][0], want)
    if "rooms_reached" in c:
        res = g.query_world_reach(cells=np.array(list(itertools.product((-5, 4), repeat=3))))
        assert int((res["status"] == 0).sum()) == c["rooms_reached"] and int((res["status"] == 1).sum()) == 8 - c["rooms_reached"]
    if "marks" in c:   # the cell across the corner falls to 564 only if c's brick wakes d's
        assert g.query_world_reach(cells=np.array(c["marks"]))["cost"].tolist() == [550, 560, 560, 564]
    if "lonely" in c:  # nothing crosses the coordinate range
        assert info["n_reached"] == 512 * len(c["lonely"]) and info["n_traversable"] == 2 * info["n_reached"]
        res = g.query_world_reach(cells=np.array(c["lonely"]) * 8)
        assert (res["status"] == 1).all() and (res["cost"] == NO).all()
    if name.startswith("shell"):
        assert g.query_world_reach(cells=[(4, 4, 4)])["status"][0] == 3
    if name.startswith("plate"):
        assert info["n_bricks"] == 2116 and info["n_reached"] == 46 * 46 * 64
    if name == "corridor":
        assert info["rounds"] > 8 and info["max_cost_reached"] == 950 and g.world_reach_bricks_relaxed() >= 12
    g.close()


# ---- 6: random, every combination of the class flags and the inflation, a budget, a box
def test_the_random_archive_under_every_option():
    hdr, cells = wc.random_world()
    c = dict(hdr=hdr, cells=cells, starts=np.array(wc.RANDOM_STARTS), kw={})
    g = world_of(c)
    seen = set()
    for kw in wc.random_variants():
        (coords, cost, info), ref = check_build(g, c, n_goals=12, **kw)
        seen.add((int(info["flags"]), int(info["inflate"])))
        assert info["n_starts_used"] <= 2
        if kw.get("max_cost"):
            assert 0 < info["max_cost_reached"] <= kw["max_cost"] and (ref.trav & (ref.cost == NO)).any()
        if kw.get("box"):
            assert 0 < info["n_bricks"] < len(hdr)
    assert len(seen) >= 24
    g.close()


# ---- 9: the build is a snapshot
def answers(g, goals):
    coords, cost, info = g.world_reach()
    rows, lens = g.world_reach_paths(cells=goals, max_len=40)
    return [coords.tobytes(), cost.tobytes(), info.tobytes(), g.query_world_reach(cells=goals).tobytes(), rows.tobytes(), lens.tobytes()]


def test_the_build_is_a_snapshot():
    hdr, cells = wc.random_world()
    c = dict(hdr=hdr, cells=cells, starts=np.array(wc.RANDOM_STARTS), kw=dict(through_unknown=True, ignore_movable=True))
    g = world_of(c)
    _, ref = check_build(g, c)
    goals = wc.sample_goals(ref, 16, seed=3)
    before = answers(g, goals)
    assert g.world_retain(bmin=(0, -1, 0), bmax=(5, 5, 5)) > 0          # removes bricks and compacts the pool
    assert answers(g, goals) == before
    other = wc.pillars(1, False)
    g.world_import(other["hdr"], other["cells"], offset=(3, 0, -5))
    assert answers(g, goals) == before
    g.world_clear()
    assert answers(g, goals) == before
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        g.world_reach_update(start_cells=c["starts"])
    assert answers(g, goals) == before                                   # (a refused build leaves the last one standing)
    g.world_import(other["hdr"], other["cells"])                       # a new build sees the new archive
    check_build(g, other)
    g.close()


# ---- 10: starts
def test_starts():
    c = wc.pillars(0, False)
    g = world_of(c)
    ref0 = wrr.DenseField(c["hdr"], c["cells"], c["starts"], MM, through_unknown=True)
    at = np.argwhere(~ref0.trav)[0]
    wall = ref0.coords[at[0]].astype(np.int64) * 8 + [at[1] & 7, (at[1] >> 3) & 7, at[1] >> 6]
    good = c["starts"]
    sets = {"duplicates": np.concatenate([good, good, good[:1]]), "on an obstacle": np.array([wall]), "in no brick": np.array([[-4, 4, 4], [900, 0, 0]]),
            "out of range": np.array([[1 << 20, 0, 0], [0, -(1 << 19) - 8, 0]]), "mixed": np.concatenate([[wall], good[1:], [[-4, 4, 4]]]),
            "none": np.zeros((0, 3), np.int64)}
    for name, starts in sets.items():
        case = dict(c, starts=starts)
        (coords, cost, info), ref = check_build(g, case, n_goals=6)
        used = {"duplicates": 2, "mixed": 1}.get(name, 0)
        assert info["n_starts_used"] == used and (info["n_reached"] > 0) == (used > 0), name
        if not used:
            assert (cost == NO).all() and info["max_cost_reached"] == 0 and info["rounds"] == 0
    # as points: the same field; non-finite and far points are ignored
    xyz = np.concatenate([wrr.cell_centres(good, SIZE), np.array([[np.nan, 0, 0], [0, np.inf, 0], [1e30, 0, 0], [-3e38, 0, 0]], np.float32)])
    g.world_reach_update(start_cells=good, through_unknown=True)
    by_cells = g.world_reach()
    g.world_reach_update(starts=xyz, through_unknown=True)
    by_points = g.world_reach()
    assert by_points[1].tobytes() == by_cells[1].tobytes() and by_points[2]["n_starts_used"] == 2
    special = np.array([[np.nan, 0, 0], [0, -np.inf, 0], [1e30, 0, 0], [2.1e6, 0, 0]], np.float32)
    res = g.query_world_reach(xyz=special)
    assert wrr.equal_results(res, ref0.query(SIZE, xyz=special)) is None and (res["status"] == 3).all() and (res["cell"] == 0).all()
    g.close()


def test_an_empty_field_is_no_error():
    """a box that holds no brick, and an archive that a retain has emptied: a field of no bricks, every goal in no brick"""
    c = wc.one_brick((2, -3, 4))
    goals = np.concatenate([c["starts"], [[0, 0, 0]]])
    for empty_archive in (False, True):
        g = world_of(c)
        if empty_archive:
            assert g.world_retain(bmin=(0, 0, 0), bmax=(-1, 0, 0)) == 1 and g.world_info()["n_bricks"] == 0
            g.world_reach_update(start_cells=c["starts"])
        else:
            g.world_reach_update(start_cells=c["starts"], box=((100, 100, 100), (101, 101, 101)))
        coords, cost, info = g.world_reach()
        assert coords.shape == (0, 3) and cost.shape == (0, 512)
        assert all(info[k] == 0 for k in ("n_bricks", "n_starts_used", "n_traversable", "n_reached", "max_cost_reached", "rounds"))
        res = g.query_world_reach(cells=goals)
        assert (res["status"] == 3).all() and (res["cost"] == NO).all() and (res["next"] == 255).all() and np.array_equal(res["cell"], goals)
        rows, lens = g.world_reach_paths(cells=goals, max_len=3)
        assert (lens == 0).all() and (rows == FILL).all()
        if not empty_archive:   # the next build, without the box, has the brick again
            check_build(g, c)
        g.close()


# ---- 11: device mode, canaries, short rows
def test_device_mode_equals_host_mode_and_nothing_is_written_beyond():
    c = crafted("pillars inflate=1 face=False")
    g = world_of(c)
    _, ref = check_build(g, c)
    goals = wc.sample_goals(ref, 40, seed=9).astype(np.int32)
    n = len(goals)
    xyz = wrr.cell_centres(goals, SIZE)
    host = g.query_world_reach(cells=goals)
    paths = ref.paths(SIZE, cells=goals)
    longest = max(len(p) for p in paths)
    assert longest > 6
    CAN = 0xA5
    for max_len in (longest, 5, 0):
        rows_h, lens_h = g.world_reach_paths(cells=goals, max_len=max_len)
        assert lens_h.tolist() == [len(p) for p in paths]                # the true lengths, whatever max_len
        for row, p in zip(rows_h, paths):
            k = min(len(p), max_len)
            assert np.array_equal(row[:k], p[:k]) and (row[k:] == FILL).all()   # the rest of a row is left untouched
        for d_in, kw in ((g.device_put(goals), "cells"), (g.device_put(xyz), "xyz")):
            d_out = g.device_put(np.full(n * 24 + 16, CAN, np.uint8))    # 8 bytes of canary before and behind
            d_rows = g.device_put(np.full(n * max_len * 12 + 16, CAN, np.uint8))
            d_lens = g.device_put(np.full(n * 4 + 16, CAN, np.uint8))
            g.query_world_reach(**{kw: d_in}, on_device=True, n=n, out=d_out + 8)
            g.world_reach_paths(**{kw: d_in}, max_len=max_len, on_device=True, n=n, cells_out=d_rows + 8, len_out=d_lens + 8)
            g.synchronize()
            out = g.device_download(d_out, n * 24 + 16)
            assert (out[:8] == CAN).all() and (out[-8:] == CAN).all() and out[8:-8].tobytes() == host.tobytes()
            lens = g.device_download(d_lens, n * 4 + 16)
            assert (lens[:8] == CAN).all() and (lens[-8:] == CAN).all() and lens[8:-8].tobytes() == lens_h.tobytes()
            rows = g.device_download(d_rows, n * max_len * 12 + 16)
            assert (rows[:8] == CAN).all() and (rows[-8:] == CAN).all()
            rows = rows[8:-8].view(np.int32).reshape(n, max_len, 3)
            for row, p in zip(rows, paths):
                k = min(len(p), max_len)
                assert np.array_equal(row[:k], p[:k]) and (row[k:].view(np.uint8) == CAN).all()
            for p in (d_in, d_out, d_rows, d_lens):
                g.device_free(p)
    # host mode, canaries behind the getter's and the queries' buffers
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    coords, cost, info = g.world_reach()
    nb, got = len(coords), C.c_int64()
    first, cap = 2, nb - 5
    assert cap > 2
    cb, wb = np.full((cap + 2, 3), 0x5A5A, np.int16), np.full((cap + 2, 512), 0xA5A5A5A5, np.uint32)
    assert L.sdm_get_world_reach(h, vp(cb), vp(wb), first, cap, C.byref(got), None) == 0 and got.value == nb
    assert np.array_equal(cb[:cap], coords[first:first + cap]) and np.array_equal(wb[:cap], cost[first:first + cap])
    assert (cb[cap:] == 0x5A5A).all() and (wb[cap:] == 0xA5A5A5A5).all()
    assert L.sdm_get_world_reach(h, vp(cb), vp(wb), nb + 3, cap, C.byref(got), None) == 0 and np.array_equal(cb[:cap], coords[first:first + cap])
    part = g.world_reach(first=3, cap=4)
    assert np.array_equal(part[0], coords[3:7]) and np.array_equal(part[1], cost[3:7]) and g.world_reach(with_cost=False)[1] is None
    out = np.full((n + 1) * 24, CAN, np.uint8)
    assert L.sdm_query_world_reach(h, None, vp(goals), n, vp(out), 0) == 0 and (out[n * 24:] == CAN).all() and out[:n * 24].tobytes() == host.tobytes()
    g.close()


# ---- 12: two runs, no side effects
def test_two_runs_give_the_same_bytes_and_the_map_is_left_alone():
    cfg = sc.config("B")
    g = twg.crafted(cfg, sc.crafted_steps(cfg), seed=12)
    g.world_update()
    state = lambda: [a.tobytes() for a in g.world_bricks()] + [g.world_info().tobytes(), g.voxels().tobytes(), repr(g.ring_state())]  # noqa: E731
    before = state()
    hdr, cells = g.world_bricks()
    ref = wrr.DenseField(hdr, cells, np.zeros((0, 3)), cfg["max_movable_track"], through_unknown=True, ignore_movable=True)
    at = np.argwhere(ref.trav)
    starts = ref.coords[at[::97, 0]].astype(np.int64) * 8 + np.stack([at[::97, 1] & 7, (at[::97, 1] >> 3) & 7, at[::97, 1] >> 6], 1)
    runs = []
    for _ in range(2):
        g.world_reach_update(start_cells=starts, through_unknown=True, ignore_movable=True)
        goals = wc.sample_goals(ref, 30, seed=1)
        runs.append(answers(g, goals))
    assert runs[0][2] != b"" and runs[0][:2] == runs[1][:2] and runs[0][3:] == runs[1][3:]
    i0, i1 = np.frombuffer(runs[0][2], binding.WORLD_REACH_INFO)[0], np.frombuffer(runs[1][2], binding.WORLD_REACH_INFO)[0]
    assert all(i0[k] == i1[k] for k in binding.WORLD_REACH_INFO.names if k != "rounds") and i0["n_reached"] > 0
    assert state() == before
    g.close()


# ---- 13: frames, world_update and a camera that leaves what it archived
def test_a_route_back_to_what_the_block_has_left():
    cfg = sc.config("B")
    N, size = twg.dims(cfg), np.float32(cfg["voxel_size"])
    rng = np.random.default_rng(4)
    u = rng.random(tuple(N[::-1]))
    occ = np.zeros(tuple(N[::-1]), np.int8)
    occ[u < 0.08] = -1
    occ[u < 0.04] = 1
    drive = int(N[2]) // 4
    occ[int(N[2]) // 2 + drive - 3:int(N[2]) // 2 + drive + 4, int(N[1]) // 2 - 3:int(N[1]) // 2 + 3, :] = 0   # free where the camera will stand
    steps = np.array(sc.crafted_steps(cfg), np.int64)
    ring = sc.crafted_ring(cfg, steps)
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    n_occ = int((occ == 1).sum())
    g.load_state(sc.crafted_state(cfg, ring, _cells(occ == 1), _cells(occ == -1), tracks=np.full(n_occ, 65535), labels=np.full(n_occ, 8)))
    g.set_ring_state(ring)
    twg.blind_frame(g, cfg, ring["last_pos"])
    g.world_update()
    for _ in range(2):                                   # the camera drives off along z; what comes in is unobserved
        steps[2] += drive // 2
        twg.blind_frame(g, cfg, twg.cam_of(cfg, steps))
        g.world_update()
    assert g.ring_state()["moved_steps"] == steps.tolist()
    cam = twg.cam_of(cfg, steps)
    hdr, cells = g.world_bricks()
    kw = dict(through_unknown=True)
    g.world_reach_update(starts=[cam], **kw)
    start = wrr.cells_of_points([cam], size)[0]
    ref = wrr.DenseField(hdr, cells, start, cfg["max_movable_track"], stamp=int(g.world_info()["stamp"]), **kw)
    got = g.world_reach()
    assert wrr.equal_fields(got, ref) is None, wrr.equal_fields(got, ref)
    assert got[2]["n_starts_used"] == 1 and got[2]["stamp"] == g.ring_state()["global_time_stamp"]
    goals = wc.sample_goals(ref, 60, seed=2)
    want = check_goals(g, ref, goals, size)
    g0 = steps - (N >> 1)                                # world cell of the block's cell (0, 0, 0)
    outside = ((goals < g0) | (goals >= g0 + N)).any(axis=1)
    assert int(((want["status"] == 0) & outside).sum()) > 0
    g.close()


# ---- 14: the argument checks
def test_argument_errors():
    g = handle()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o, info = np.zeros(1, binding.WORLD_REACH_OPTIONS), np.zeros(1, binding.WORLD_REACH_INFO)
    p, w = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32)
    res, lens, rows = np.zeros(2, binding.WORLD_REACH_RESULT), np.zeros(2, np.int32), np.zeros((2, 4, 3), np.int32)
    got = C.c_int64(-7)
    # before the archive has had an update or import; the getter and the queries before any build
    assert L.sdm_world_reach_update(h, vp(o), vp(p), None, 2) == INV and b"sdm_world_update first" in L.sdm_last_error()
    c = wc.one_brick((0, 0, 0))
    g.world_import(c["hdr"], c["cells"])
    assert L.sdm_get_world_reach(h, None, None, 0, 0, C.byref(got), vp(info)) == INV and b"sdm_world_reach_update first" in L.sdm_last_error()
    assert L.sdm_query_world_reach(h, vp(p), None, 2, vp(res), 0) == INV and L.sdm_world_reach_paths(h, vp(p), None, 2, 4, vp(rows), vp(lens), 0) == INV
    assert got.value == -7
    # the build's arguments
    assert L.sdm_world_reach_update(h, None, vp(p), None, 2) == INV
    assert L.sdm_world_reach_update(h, vp(o), None, None, 0) == INV and L.sdm_world_reach_update(h, vp(o), vp(p), vp(w), 2) == INV
    assert L.sdm_world_reach_update(h, vp(o), vp(p), None, -1) == INV
    for field, bad in (("flags", 0x10), ("inflate", 3), ("pad", 1)):
        o[field] = bad
        assert L.sdm_world_reach_update(h, vp(o), vp(p), None, 2) == INV, field
        o[field] = 0
    o["flags"], o["bmin"], o["bmax"] = binding.WORLD_REACH_BOX, (0, 0, 0), (0, -1, 0)
    assert L.sdm_world_reach_update(h, vp(o), vp(p), None, 2) == INV and b"bmax" in L.sdm_last_error()
    o["flags"] = 0                                      # without the flag the box is not read
    assert L.sdm_world_reach_update(h, vp(o), vp(p), None, 2) == 0 and L.sdm_world_reach_update(h, vp(o), None, vp(w), 0) == 0
    # the getter and the queries
    assert L.sdm_get_world_reach(h, None, None, 0, 0, C.byref(got), vp(info)) == 0 and got.value == 1 and info["n_starts_used"][0] == 0
    assert L.sdm_get_world_reach(h, None, None, -1, 0, C.byref(got), None) == INV and L.sdm_get_world_reach(h, None, None, 0, -1, C.byref(got), None) == INV
    assert L.sdm_get_world_reach(h, None, None, 0, 0, None, vp(info)) == INV
    assert L.sdm_query_world_reach(h, None, None, 2, vp(res), 0) == INV and L.sdm_query_world_reach(h, vp(p), vp(w), 2, vp(res), 0) == INV
    assert L.sdm_query_world_reach(h, vp(p), None, -1, vp(res), 0) == INV and L.sdm_query_world_reach(h, vp(p), None, 2, None, 0) == INV
    assert L.sdm_query_world_reach(h, vp(p), None, 2, vp(res), 4) == INV and L.sdm_query_world_reach(h, vp(p), None, 0, vp(res), 0) == 0
    assert L.sdm_world_reach_paths(h, None, None, 2, 4, vp(rows), vp(lens), 0) == INV and L.sdm_world_reach_paths(h, vp(p), vp(w), 2, 4, vp(rows), vp(lens), 0) == INV
    assert L.sdm_world_reach_paths(h, vp(p), None, 2, -1, vp(rows), vp(lens), 0) == INV and L.sdm_world_reach_paths(h, vp(p), None, 2, 4, None, vp(lens), 0) == INV
    assert L.sdm_world_reach_paths(h, vp(p), None, 2, 4, vp(rows), None, 0) == INV and L.sdm_world_reach_paths(h, vp(p), None, -2, 4, vp(rows), vp(lens), 0) == INV
    assert L.sdm_world_reach_paths(h, vp(p), None, 2, 4, vp(rows), vp(lens), 8) == INV and L.sdm_world_reach_paths(h, vp(p), None, 2, 0, None, vp(lens), 0) == 0
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert L.sdm_world_reach_update(shard.h, vp(o), vp(p), None, 2) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_get_world_reach(shard.h, None, None, 0, 0, C.byref(got), None) == INV
    assert L.sdm_query_world_reach(shard.h, vp(p), None, 2, vp(res), 0) == INV
    assert L.sdm_world_reach_paths(shard.h, vp(p), None, 2, 4, vp(rows), vp(lens), 0) == INV
    shard.close()
