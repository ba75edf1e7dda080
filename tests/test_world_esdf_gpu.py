"""sdm_world_esdf_update / sdm_get_world_esdf / sdm_query_world_distance (include/sdm.h) against tests/world_esdf_ref.py's
BrickModel, bit for bit: coords, d2, offset and info.  The model is fed with what world_bricks() of the same map returns.

The archive needs a map only as a handle: every case but the last feeds the hand-written bricks of
tests/world_esdf_cases.py to world_import on a fresh map of shape A (4 cells an axis).  The crafted cases with their closed
forms, the random archive under every flag combination and radius without and with a box, empty fields; queries by points
and by cells in host and device mode; the ranges of the getter; the snapshot under retain, import and clear;
reproducibility and no side effects; a build after a larger one; the argument checks; frames whose camera leaves what it
archived, the distance field and world reach together."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import test_world_gpu as twg
from tests import world_esdf_cases as ec
from tests import world_esdf_ref as wer
from tests.test_ground_gpu import _cells
from tests.test_world_esdf_ref import check_closed_forms, check_random

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV = 1
CFG = ec.CFG
SIZE = np.float32(CFG["voxel_size"])
MM = ec.MM
NONE, FAR, NO_BRICK = ec.NONE, binding.WORLD_ESDF_FAR, 0xFFFFFFFF


def handle():
    return binding.SdmMap(CFG, PARAMS, synth.noise_table())


def world_of(c):
    g = handle()
    g.world_import(c["hdr"], c["cells"])
    return g


def check_build(g, max_movable=MM, **kw):
    """one build on the map and in the restatement, fed with what the map itself returns"""
    hdr, cells = g.world_bricks()
    g.world_esdf_update(**kw)
    ref = wer.BrickModel(hdr, cells, max_movable=max_movable, stamp=int(g.world_info()["stamp"]), **kw)
    diff = wer.difference(g.world_esdf(), wer.answer(ref))
    assert diff is None, diff
    return ref


def field_bytes(g):
    return [np.asarray(a).tobytes() for a in g.world_esdf()]


CASES = None


def crafted(name):
    global CASES
    CASES = CASES or ec.crafted()
    return CASES[name]


# ---- 1 - 8: the crafted cases
@pytest.mark.parametrize("name", sorted(ec.crafted()))
def test_crafted_archives(name):
    c = crafted(name)
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    check_closed_forms(name, ref)     # (the library's answer is the model's, bit for bit)
    g.close()


# ---- 9: random, every flag combination x radius, without and with a box
def test_the_random_archive_under_every_option():
    hdr, cells = ec.random_archive()
    g = world_of(dict(hdr=hdr, cells=cells))
    seen = set()
    for kw in ec.random_variants():
        ref = check_build(g, **kw)
        check_random(ref, kw)
        seen.add((int(ref.info["flags"]), int(ref.info["radius"])))
    assert len(seen) == 40
    g.close()


# ---- 10: empty fields
def test_an_empty_field_is_no_error():
    c = crafted("x wrap")
    for empty_archive in (False, True):
        g = world_of(c)
        if empty_archive:
            assert g.world_retain(bmin=(0, 0, 0), bmax=(-1, 0, 0)) == 1 and g.world_info()["n_bricks"] == 0
            boxes = [None]
        else:
            boxes = [((100, 100, 100), (101, 101, 101)), ((0, 0, 0), (0, -1, 0))]
        for box in boxes:
            check_build(g, radius=8, box=box)
            coords, d2, offset, info = g.world_esdf()
            assert coords.shape == (0, 3) and d2.shape == (0, 512) and offset.shape == (0, 512, 3)
            assert all(info[k] == 0 for k in ("n_bricks", "n_obstacle_cells", "n_near_cells")) and info["radius"] == 8
            res = g.query_world_distance(cells=[(0, 3, 4)])
            assert res["d2"][0] == NO_BRICK and res["distance"][0] == -1.0
        if not empty_archive:   # the next build, without the box, has the brick again
            assert check_build(g, radius=8).info["n_near_cells"] > 0
        g.close()


# ---- queries: points and cells, host and device mode
def test_queries_by_points_and_cells_in_host_and_device_mode():
    c = crafted("far 16 x")
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    rng = np.random.default_rng(6)
    inside = np.stack([rng.integers(-16, 24, 60), rng.integers(0, 8, 60), rng.integers(0, 8, 60)], 1)
    special = np.array([(0, 3, 3), (1, 3, 3), (7, 3, 3), (-16, 3, 3), (23, 3, 3), (-17, 3, 3), (24, 0, 0), (0, 8, 0), (0, 0, -1), (0, 3, 40),
                        (1 << 30, 0, 0), (0, -(1 << 30), 5), (262144 * 8, 0, 0)], np.int64)
    cells = np.concatenate([special, inside]).astype(np.int32)
    want = ref.query(cells, SIZE)
    assert (want["d2"] == FAR).any() and (want["d2"] == NO_BRICK).any() and (want["d2"] == 256).any() and (want["d2"] == 0).sum() >= 2
    host = g.query_world_distance(cells=cells)
    assert host.tobytes() == want.tobytes()
    far = host[host["d2"] == FAR]
    assert (far["distance"] == np.sqrt(np.float32(257)) * SIZE).all() and np.array_equal(far["nearest"], far["cell"])
    # by points: the centres of the cells that a float32 can hold, a NaN, an infinity and two points beyond the brick range
    ok = (np.abs(cells.astype(np.int64)) < (1 << 20)).all(axis=1)
    xyz = ((cells[ok].astype(np.float32) + np.float32(0.5)) * SIZE).astype(np.float32)
    bad = np.array([(np.nan, 0, 0), (0, np.inf, 0), (3e9, 0, 0), (0, 0, -262145.0)], np.float32)
    pts = np.concatenate([xyz, bad])
    want_p = np.concatenate([want[ok], np.zeros(len(bad), binding.WORLD_DISTANCE_RESULT)])
    want_p["d2"][-len(bad):], want_p["distance"][-len(bad):] = NO_BRICK, -1.0      # cell and nearest (0, 0, 0)
    host_p = g.query_world_distance(xyz=pts)
    assert host_p.tobytes() == want_p.tobytes()
    CAN = 0xA5
    for src, expect, kw in ((cells, host, "cells"), (pts, host_p, "xyz")):
        n = len(src)
        d_in = g.device_put(src)
        d_out = g.device_put(np.full(n * 32 + 16, CAN, np.uint8))     # 8 bytes of canary before and behind
        g.query_world_distance(**{kw: d_in}, on_device=True, n=n, out=d_out + 8)
        g.synchronize()
        out = g.device_download(d_out, n * 32 + 16)
        assert (out[:8] == CAN).all() and (out[-8:] == CAN).all() and out[8:-8].tobytes() == expect.tobytes()
        g.device_free(d_in), g.device_free(d_out)
    # host mode writes nothing behind its n results; n == 0 is fine
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full((len(cells) + 1) * 32, CAN, np.uint8)
    assert L.sdm_query_world_distance(h, None, vp(cells), len(cells), vp(out), 0) == 0
    assert (out[len(cells) * 32:] == CAN).all() and out[:len(cells) * 32].tobytes() == host.tobytes()
    assert L.sdm_query_world_distance(h, None, vp(cells), 0, vp(out), 0) == 0 and (out[len(cells) * 32:] == CAN).all()
    g.close()


# ---- the ranges of the getter
def test_getter_ranges_and_canaries():
    c = crafted("pillars static_only=False")
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    n = len(ref.coords)
    assert n == 17
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = C.c_int64(-1)
    for first, cap in ((0, n), (3, 5), (n - 2, 6), (n, 4), (n + 5, 4), (2, 0)):
        take = max(min(n - first, cap), 0)
        cb, db, ob = np.full((cap + 2, 3), 0x5A5A, np.int16), np.full((cap + 2, 512), 0xA5A5, np.uint16), np.full((cap + 2, 512, 3), 0x5A, np.int8)
        assert L.sdm_get_world_esdf(h, vp(cb), vp(db), vp(ob), first, cap, C.byref(got), None) == 0 and got.value == n
        assert np.array_equal(cb[:take], ref.coords[first:first + take]) and (cb[take:] == 0x5A5A).all()
        assert np.array_equal(db[:take], ref.d2[first:first + take]) and (db[take:] == 0xA5A5).all()
        assert np.array_equal(ob[:take], ref.offset[first:first + take]) and (ob[take:] == 0x5A).all()
    part = g.world_esdf(first=4, cap=6)
    assert np.array_equal(part[0], ref.coords[4:10]) and np.array_equal(part[1], ref.d2[4:10]) and np.array_equal(part[2], ref.offset[4:10])
    # each array alone, and none
    db = np.zeros((n, 512), np.uint16)
    assert L.sdm_get_world_esdf(h, None, vp(db), None, 0, n, C.byref(got), None) == 0 and np.array_equal(db, ref.d2)
    ob = np.zeros((n, 512, 3), np.int8)
    assert L.sdm_get_world_esdf(h, None, None, vp(ob), 0, n, C.byref(got), None) == 0 and np.array_equal(ob, ref.offset)
    cb = np.zeros((n, 3), np.int16)
    assert L.sdm_get_world_esdf(h, vp(cb), None, None, 0, n, C.byref(got), None) == 0 and np.array_equal(cb, ref.coords)
    info = np.zeros(1, binding.WORLD_ESDF_INFO)
    assert L.sdm_get_world_esdf(h, None, None, None, 0, n, C.byref(got), vp(info)) == 0 and got.value == n and info.tobytes() == ref.info.tobytes()
    # without a box row r is row r of world_bricks()
    hdr, _ = g.world_bricks()
    assert np.array_equal(ref.coords, np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int16))
    g.close()


# ---- the build is a snapshot
def test_the_build_is_a_snapshot():
    hdr, cells = ec.random_archive()
    g = world_of(dict(hdr=hdr, cells=cells))
    ref = check_build(g, radius=9, static_only=True)
    probes = np.array([(0, 0, 0), (-16, 3, 3), (18, 18, 18), (100, 0, 0)], np.int32)
    before, asked = field_bytes(g), g.query_world_distance(cells=probes).tobytes()
    assert asked == ref.query(probes, SIZE).tobytes()
    assert g.world_retain(bmin=(0, -1, 0), bmax=(5, 5, 5)) > 0          # removes bricks and compacts the pool
    assert field_bytes(g) == before and g.query_world_distance(cells=probes).tobytes() == asked
    other = crafted("far diagonal")
    g.world_import(other["hdr"], other["cells"], offset=(3, 0, -5))
    assert field_bytes(g) == before
    g.world_clear()
    assert field_bytes(g) == before and g.query_world_distance(cells=probes).tobytes() == asked
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        g.world_esdf_update(radius=4)
    assert field_bytes(g) == before                                     # (a refused build leaves the last one standing)
    g.world_import(other["hdr"], other["cells"])                        # a new build sees the new archive
    check_build(g, **other["kw"])
    g.close()


# ---- two runs, no side effects
def test_two_runs_give_the_same_bytes_and_the_map_is_left_alone():
    cfg = sc.config("B")
    g = twg.crafted(cfg, sc.crafted_steps(cfg), seed=12)
    g.world_update()
    state = lambda: [a.tobytes() for a in g.world_bricks()] + [g.world_info().tobytes(), g.voxels().tobytes(), repr(g.ring_state())]  # noqa: E731
    before = state()
    runs = []
    for _ in range(2):
        ref = check_build(g, max_movable=cfg["max_movable_track"], radius=9, static_only=True)
        runs.append(field_bytes(g))
    assert runs[0] == runs[1] and ref.info["n_near_cells"] > ref.info["n_obstacle_cells"] > 0
    assert ref.info["stamp"] == g.ring_state()["global_time_stamp"]
    assert state() == before
    g.close()


# ---- a build after a larger one: the buffers were grown, then are reused
def test_a_smaller_build_after_a_larger_one():
    hdr, cells = ec.random_archive()
    g = world_of(dict(hdr=hdr, cells=cells))
    small = crafted("x wrap")
    check_build(g, radius=3)
    big = check_build(g, radius=16, unknown_is_obstacle=True)
    assert big.info["n_bricks"] == 122
    check_build(g, radius=16, box=ec.RANDOM_BOX)                        # fewer bricks, the same archive
    g.world_clear()
    g.world_import(small["hdr"], small["cells"])                        # fewer archived bricks
    ref = check_build(g, **small["kw"])
    check_closed_forms("x wrap", ref)
    res = g.query_world_distance(cells=[(-16, 3, 3)])                   # a brick of the larger build's table
    assert res["d2"][0] == NO_BRICK
    g.world_import(hdr, cells)                                          # ... and more again
    check_build(g, radius=8, static_only=True)
    g.close()


# ---- integration: frames, world_update, the distance field and world reach from the camera
def test_a_path_through_the_archive_keeps_its_clearance():
    cfg = sc.config("B")
    N = twg.dims(cfg)
    rng = np.random.default_rng(4)
    u = rng.random(tuple(N[::-1]))
    occ = np.zeros(tuple(N[::-1]), np.int8)
    occ[u < 0.03] = -1
    occ[u < 0.003] = 1
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
    cam = twg.cam_of(cfg, steps)
    ref = check_build(g, max_movable=cfg["max_movable_track"], radius=8)
    g.world_reach_update(starts=[cam], inflate=2, through_unknown=True)
    coords, cost, info = g.world_reach()
    assert info["n_starts_used"] == 1 and np.array_equal(coords, ref.coords)      # the same bricks, the same order
    w = np.arange(512)
    cells = coords.astype(np.int64)[:, None, :] * 8 + np.stack([w & 7, (w >> 3) & 7, w >> 6], 1)[None]
    g0 = steps - (N >> 1)                                # world cell of the block's cell (0, 0, 0)
    outside = ((cells < g0) | (cells >= g0 + N)).any(axis=2)
    reached = (cost != 0xFFFFFFFF) & outside
    assert reached.any()
    r, k = np.unravel_index(np.argmax(np.where(reached, cost, 0)), cost.shape)      # the farthest reached cell beyond the block
    goal = cells[r, k][None]
    rows, lens = g.world_reach_paths(cells=goal, max_len=int(cost[r, k]) // 10 + 1)
    assert lens[0] > 8 and rows[0, 0].tolist() == goal[0].tolist()
    path = g.query_world_distance(cells=rows[0, :lens[0]])
    print("clearance along the path: d2", sorted(set(path["d2"].tolist()))[:8])
    # an obstacle within Euclidean 2 is within Chebyshev 2, which the inflation excludes
    assert (path["d2"] > 4).all() and (path["d2"] != NO_BRICK).all()
    # ... and every field cell with d2 <= 4 reads not traversable in the reach field
    close = cells[ref.d2 <= 4]
    assert len(close) > 100
    assert (g.query_world_reach(cells=close)["status"] == 2).all()
    g.close()


# ---- the argument checks
def test_argument_errors():
    g = handle()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o, info = np.zeros(1, binding.WORLD_ESDF_OPTIONS), np.zeros(1, binding.WORLD_ESDF_INFO)
    o["radius"] = 4
    out, cells, xyz = np.zeros(2, binding.WORLD_DISTANCE_RESULT), np.zeros((2, 3), np.int32), np.zeros((2, 3), np.float32)
    k64 = C.c_int64(-7)
    # before the archive has had an update or import; the getter and the query before any build
    assert L.sdm_world_esdf_update(h, vp(o)) == INV and b"sdm_world_update first" in L.sdm_last_error()
    c = crafted("x wrap")
    g.world_import(c["hdr"], c["cells"])
    assert L.sdm_get_world_esdf(h, None, None, None, 0, 0, C.byref(k64), vp(info)) == INV and b"sdm_world_esdf_update first" in L.sdm_last_error()
    assert L.sdm_query_world_distance(h, None, vp(cells), 2, vp(out), 0) == INV and b"sdm_world_esdf_update first" in L.sdm_last_error()
    assert k64.value == -7
    # the build's arguments
    assert L.sdm_world_esdf_update(h, None) == INV
    o["flags"] = 0x8
    assert L.sdm_world_esdf_update(h, vp(o)) == INV and b"flag" in L.sdm_last_error()
    o["flags"] = 0
    for bad in (0, 17, 0xFFFFFFFF):
        o["radius"] = bad
        assert L.sdm_world_esdf_update(h, vp(o)) == INV and b"radius" in L.sdm_last_error()
    o["radius"], o["bmin"], o["bmax"] = 16, (5, 5, 5), (4, 4, 4)          # without the flag the box is not read
    assert L.sdm_world_esdf_update(h, vp(o)) == 0
    # the getter
    assert L.sdm_get_world_esdf(h, None, None, None, 0, 0, C.byref(k64), vp(info)) == 0 and k64.value == 1 and info["radius"][0] == 16
    assert L.sdm_get_world_esdf(h, None, None, None, -1, 0, C.byref(k64), None) == INV and L.sdm_get_world_esdf(h, None, None, None, 0, -1, C.byref(k64), None) == INV
    assert L.sdm_get_world_esdf(h, None, None, None, 0, 0, None, None) == INV
    # the query
    assert L.sdm_query_world_distance(h, None, None, 0, vp(out), 0) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_query_world_distance(h, vp(xyz), vp(cells), 2, vp(out), 0) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_query_world_distance(h, vp(xyz), None, -1, vp(out), 0) == INV and L.sdm_query_world_distance(h, vp(xyz), None, 2, None, 0) == INV
    assert L.sdm_query_world_distance(h, vp(xyz), None, 2, vp(out), 0x80) == INV
    assert L.sdm_query_world_distance(h, vp(xyz), None, 2, vp(out), 0) == 0
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    o[:] = 0
    o["radius"] = 4
    assert L.sdm_world_esdf_update(shard.h, vp(o)) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_get_world_esdf(shard.h, None, None, None, 0, 0, C.byref(k64), None) == INV
    assert L.sdm_query_world_distance(shard.h, vp(xyz), None, 2, vp(out), 0) == INV
    shard.close()
