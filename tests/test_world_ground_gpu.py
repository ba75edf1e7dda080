"""sdm_world_ground_update / sdm_get_world_ground / sdm_query_world_ground / sdm_query_world_footprints (include/sdm.h)
against tests/world_ground_ref.py's ColumnModel, bit for bit: coords, cells, d2, info, query and footprint results.  The
model is fed with what world_bricks() of the same map returns.

The archive needs a map only as a handle: every case but the last feeds the hand-written bricks of
tests/world_ground_cases.py to world_import on a fresh map of shape A (4 cells an axis).  The crafted cases with the values
worked out by hand, the random archive under every flag combination, two radii and three orientations, the queries in host
and device mode, the getter's ranges, the snapshot under clear and import, reproducibility, the argument checks - and the
block's own ground layer (sdm_ground_update) on a block archived once, which the world's must agree with."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import ground_ref as gr
from tests import shape_cases as sc
from tests import world_ground_cases as gc
from tests import world_ground_ref as wgr
from tests.test_ground_gpu import _cells

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV = 1
CFG = gc.CFG
SIZE = np.float32(CFG["voxel_size"])
MM = gc.MM
NONE = gc.NONE
CASES = gc.crafted()


def handle():
    return binding.SdmMap(CFG, PARAMS, synth.noise_table())


def world_of(c):
    g = handle()
    g.world_import(c["hdr"], c["cells"])
    return g


def check_build(g, max_movable=MM, **kw):
    """one build on the map and in the restatement, fed with what the map itself returns"""
    hdr, cells = g.world_bricks()
    g.world_ground_update(**kw)
    ref = wgr.ColumnModel(hdr, cells, max_movable=max_movable, stamp=int(g.world_info()["stamp"]), **kw)
    got = g.world_ground()
    diff = wgr.difference(got, wgr.answer(ref))
    assert diff is None, diff
    for a, b in zip(got, wgr.answer(ref)):
        assert np.array_equal(a, b)
    return ref


def layer_bytes(g):
    return [np.asarray(a).tobytes() for a in g.world_ground()]


# ---- the crafted cases: orientations, height seams, cell rules, steps, distances, tile existence, the int16 edge
@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_archives(name):
    c = CASES[name]
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    c["expect"](ref)                  # (the library's answer is the model's, bit for bit)
    g.close()


# ---- the random archive: every flag combination x two radii x three orientations, and a box
def test_the_random_archive_under_every_option():
    hdr, cells = gc.random_world()
    g = world_of(dict(hdr=hdr, cells=cells))
    seen = set()
    rng = np.random.default_rng(2)
    fps = np.zeros(6, binding.FOOTPRINT)
    for kw in gc.random_variants():
        ref = check_build(g, **kw)
        seen.add((int(ref.info["options"]["flags"]), kw["radius"], kw["up"]))
        probes = rng.integers(-12, 28, (24, 3)).astype(np.int32)
        assert np.array_equal(g.query_world_ground(cells=probes), ref.query(probes, SIZE))
        t = rng.random(6) * 2 * np.pi
        fps["center_u"], fps["center_v"] = rng.random(6) * 30 - 8, rng.random(6) * 30 - 8
        fps["dir_u"], fps["dir_v"], fps["half_len"], fps["half_wid"] = np.cos(t), np.sin(t), rng.random(6) * 4, rng.random(6) * 2
        assert np.array_equal(g.query_world_footprints(fps), ref.footprints(fps, SIZE))
    assert len(seen) == 16 * 2 * 3 + 1
    g.close()


# ---- the two queries: over the corner where four tiles meet, host against device mode, n = 0
def query_entries():
    inside = np.array([(i, j, k) for i in (-8, -3, -1, 0, 2, 7) for j in (-8, -1, 0, 1, 7) for k in (-5, 0, 3, 9)], np.int64)
    special = np.array([(8, 0, 0), (0, -9, 0), (-2, 1, 5), (262143, 0, 0), (262144, 0, 0), (0, -262145, 0), (1 << 30, 0, 0), (0, 0, -(1 << 31))],
                       np.int64)
    return np.concatenate([special, inside]).astype(np.int32)


def test_queries_and_footprints_in_host_and_device_mode():
    c = gc.corner_case()
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    cells = query_entries()
    want = ref.query(cells, SIZE)
    assert (want["status"] == 3).sum() >= 7 and (want["d2"] == 0).any() and (want["above"] == wgr.INT32_MIN).any()
    host = g.query_world_ground(cells=cells)
    assert np.array_equal(host, want) and host.tobytes() == want.tobytes()
    # by points: the centres of the cells a float32 holds, a NaN, an infinity and two points beyond the brick range
    ok = (np.abs(cells.astype(np.int64)) < (1 << 18)).all(axis=1)
    xyz = ((cells[ok].astype(np.float32) + np.float32(0.5)) * SIZE).astype(np.float32)
    bad = np.array([(np.nan, 0, 0), (0, np.inf, 0), (3e9, 0, 0), (0, 0, -262145.0)], np.float32)
    pts = np.concatenate([xyz, bad])
    want_p = np.concatenate([want[ok], ref.query([(1 << 30, 0, 0)] * len(bad), SIZE)])
    host_p = g.query_world_ground(xyz=pts)
    assert np.array_equal(host_p, want_p) and host_p.tobytes() == want_p.tobytes()
    fps = gc.footprint_set()
    want_f = ref.footprints(fps, SIZE)
    assert want_f["n_absent"].max() > 3000 and (want_f["n_lethal"] > 0).sum() >= 3
    host_f = g.query_world_footprints(fps)
    assert np.array_equal(host_f, want_f) and host_f.tobytes() == want_f.tobytes()
    CAN = 0xA5
    for src, expect, call, kw in ((cells, host, g.query_world_ground, "cells"), (pts, host_p, g.query_world_ground, "xyz"),
                                  (fps, host_f, g.query_world_footprints, None)):
        n = len(src)
        d_in = g.device_put(src)
        d_out = g.device_put(np.full(n * 40 + 16, CAN, np.uint8))     # 8 bytes of canary before and behind
        if kw:
            call(**{kw: d_in}, on_device=True, n=n, out=d_out + 8)
        else:
            call(d_in, on_device=True, n=n, out=d_out + 8)
        g.synchronize()
        out = g.device_download(d_out, n * 40 + 16)
        assert (out[:8] == CAN).all() and (out[-8:] == CAN).all() and out[8:-8].tobytes() == expect.tobytes()
        g.device_free(d_in), g.device_free(d_out)
    # host mode writes nothing behind its n results; n == 0 is fine
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full((len(cells) + 1) * 40, CAN, np.uint8)
    assert L.sdm_query_world_ground(h, None, vp(cells), len(cells), vp(out), 0) == 0
    assert (out[len(cells) * 40:] == CAN).all() and out[:len(cells) * 40].tobytes() == host.tobytes()
    out[:] = CAN
    assert L.sdm_query_world_ground(h, None, vp(cells), 0, vp(out), 0) == 0 and (out == CAN).all()
    assert L.sdm_query_world_footprints(h, vp(fps), 0, vp(out), 0) == 0 and (out == CAN).all()
    g.close()


# ---- entries that stand for no world cell: nothing of such an entry reaches its result, whatever its other coordinates are
def unusable_entries(size):
    """points with a NaN, an infinity and a coordinate just outside +-262144 cells beside coordinates that are fine, and
    cells whose brick is out of the int16 range beside coordinates that are fine"""
    size = np.float32(size)
    edge = np.float32(262144.5) * size
    recip = np.float32(1) / size
    assert np.floor(edge * recip) == 262144 and np.floor(-edge * recip) == -262145    # (float32, like the library's rule)
    fine = (np.array([3.5, 2.5, 1.5], np.float32) * size).tolist()
    pts = np.array([(np.nan, fine[1], fine[2]), (fine[0], np.inf, fine[2]), (fine[0], fine[1], -np.inf), (edge, fine[1], fine[2]),
                    (fine[0], -edge, fine[2]), (fine[0], fine[1], edge)], np.float32)
    cells = np.array([(262144, 2, 1), (3, -262145, 1), (3, 2, 1 << 30), (-(1 << 31), 2, 1), (3, 2, 262144)], np.int32)
    return pts, cells


def test_entries_that_stand_for_no_world_cell():
    c = gc.corner_case()
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    pts, cells = unusable_entries(SIZE)
    assert ref.query([(3, 2, 1)], SIZE)["status"][0] == 0      # (the coordinates that are fine name a column of the layer)
    none = ref.query([(1 << 30, 0, 0)], SIZE)
    assert none["status"][0] == 3
    want_c, want_p = ref.query(cells, SIZE), np.repeat(none, len(pts))
    assert want_c.tobytes() == np.repeat(none, len(cells)).tobytes()
    assert g.query_world_ground(cells=cells).tobytes() == want_c.tobytes()
    assert g.query_world_ground(xyz=pts).tobytes() == want_p.tobytes()
    g.close()


def test_a_footprint_over_an_absent_tile():
    c = gc.corner_case(skip=[(-1, 0)])
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    assert len(ref.coords) == 3
    fps = gc.footprint_set()[:4]
    want = ref.footprints(fps, SIZE)
    assert want["n_absent"][0] == 3 and want["n_cols"][0] == 9
    assert np.array_equal(g.query_world_footprints(fps), want)
    g.close()


# ---- the ranges of the getter
def test_getter_ranges_and_canaries():
    c = CASES["diagonal"]
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    n = len(ref.coords)
    assert n == 25
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = C.c_int64(-1)
    for first, cap in ((0, n), (3, 5), (n - 2, 6), (n, 4), (n + 5, 4), (2, 0)):
        take = max(min(n - first, cap), 0)
        cb, eb, db = np.full((cap + 2, 2), 0x5A5A, np.int16), np.full((cap + 2, 64, 8), 0x5A, np.uint8), np.full((cap + 2, 64), 0xA5A5, np.uint16)
        assert L.sdm_get_world_ground(h, vp(cb), vp(eb), vp(db), first, cap, C.byref(got), None) == 0 and got.value == n
        assert np.array_equal(cb[:take], ref.coords[first:first + take]) and (cb[take:] == 0x5A5A).all()
        assert eb[:take].tobytes() == ref.cells[first:first + take].tobytes() and (eb[take:] == 0x5A).all()
        assert np.array_equal(db[:take], ref.d2[first:first + take]) and (db[take:] == 0xA5A5).all()
    part = g.world_ground(first=4, cap=6)
    assert np.array_equal(part[0], ref.coords[4:10]) and np.array_equal(part[1], ref.cells[4:10]) and np.array_equal(part[2], ref.d2[4:10])
    db = np.zeros((n, 64), np.uint16)
    assert L.sdm_get_world_ground(h, None, None, vp(db), 0, n, C.byref(got), None) == 0 and np.array_equal(db, ref.d2)
    info = np.zeros(1, binding.WORLD_GROUND_INFO)
    assert L.sdm_get_world_ground(h, None, None, None, 0, n, C.byref(got), vp(info)) == 0 and got.value == n and info.tobytes() == ref.info.tobytes()
    g.close()


# ---- the build is a snapshot
def test_the_build_is_a_snapshot():
    hdr, cells = gc.random_world()
    g = world_of(dict(hdr=hdr, cells=cells))
    kw = gc.random_variants()[5]
    ref = check_build(g, **kw)
    probes = np.array([(0, 0, 0), (-7, 3, 3), (18, 18, 8), (100, 0, 0)], np.int32)
    fps = gc.footprint_set()[:3]
    before, asked, stood = layer_bytes(g), g.query_world_ground(cells=probes).tobytes(), g.query_world_footprints(fps).tobytes()
    assert asked == ref.query(probes, SIZE).tobytes()
    other = CASES["diagonal"]
    g.world_import(other["hdr"], other["cells"], offset=(3, 0, -5))
    assert layer_bytes(g) == before and g.query_world_ground(cells=probes).tobytes() == asked
    g.world_clear()
    assert layer_bytes(g) == before and g.query_world_ground(cells=probes).tobytes() == asked
    assert g.query_world_footprints(fps).tobytes() == stood
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        g.world_ground_update(**kw)
    assert layer_bytes(g) == before                                     # (a refused build leaves the last one standing)
    g.world_import(other["hdr"], other["cells"])                        # a new build sees the new archive
    check_build(g, **other["kw"])
    g.close()


# ---- two runs; a smaller build after a larger one
def test_two_runs_give_the_same_bytes_and_the_archive_is_left_alone():
    hdr, cells = gc.random_world()
    g = world_of(dict(hdr=hdr, cells=cells))
    kw = gc.random_variants()[-1]
    state = lambda: [a.tobytes() for a in g.world_bricks()] + [g.world_info().tobytes(), g.voxels().tobytes()]  # noqa: E731
    before = state()
    runs = []
    for _ in range(2):
        check_build(g, **kw)
        runs.append(layer_bytes(g))
    assert runs[0] == runs[1] and state() == before
    small = CASES["x wrap"]
    check_build(g, **gc.random_variants()[7])
    g.world_clear()
    g.world_import(small["hdr"], small["cells"])                        # fewer archived bricks, fewer tiles
    ref = check_build(g, **small["kw"])
    small["expect"](ref)
    assert g.query_world_ground(cells=[(20, 20, 3)])["status"][0] == 3  # a tile of the larger build's table
    g.world_import(hdr, cells)                                          # ... and more again
    check_build(g, **kw)
    g.close()


# ---- the argument checks
def test_argument_errors():
    g = handle()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    info = np.zeros(1, binding.WORLD_GROUND_INFO)

    def opts(**kw):
        o = np.zeros(1, binding.WORLD_GROUND_OPTIONS)
        o["up_axis"], o["up_sign"], o["radius"], o["h_hi"] = 2, 1, 4, 7
        for k, v in kw.items():
            o[k] = v
        return o

    out, fout = np.zeros(2, binding.WORLD_GROUND_RESULT), np.zeros(2, binding.WORLD_FOOTPRINT_RESULT)
    cells, xyz, fps = np.zeros((2, 3), np.int32), np.zeros((2, 3), np.float32), np.zeros(2, binding.FOOTPRINT)
    k64 = C.c_int64(-7)
    # before the archive has had an update or import; the getter and the queries before any build
    assert L.sdm_world_ground_update(h, vp(opts())) == INV and b"sdm_world_update first" in L.sdm_last_error()
    c = CASES["x wrap"]
    g.world_import(c["hdr"], c["cells"])
    assert L.sdm_get_world_ground(h, None, None, None, 0, 0, C.byref(k64), vp(info)) == INV and b"sdm_world_ground_update first" in L.sdm_last_error()
    assert L.sdm_query_world_ground(h, None, vp(cells), 2, vp(out), 0) == INV and b"sdm_world_ground_update first" in L.sdm_last_error()
    assert L.sdm_query_world_footprints(h, vp(fps), 2, vp(fout), 0) == INV and b"sdm_world_ground_update first" in L.sdm_last_error()
    assert k64.value == -7
    # the build's arguments
    assert L.sdm_world_ground_update(h, None) == INV
    assert L.sdm_world_ground_update(h, vp(opts(flags=0x20))) == INV and b"flag" in L.sdm_last_error()
    for bad in (dict(up_axis=3), dict(up_axis=-1), dict(up_sign=0), dict(up_sign=2)):
        assert L.sdm_world_ground_update(h, vp(opts(**bad))) == INV and b"up_axis" in L.sdm_last_error()
    for bad in (dict(h_lo=8), dict(h_lo=0, h_hi=4096), dict(h_lo=-(1 << 31), h_hi=(1 << 31) - 1)):
        assert L.sdm_world_ground_update(h, vp(opts(**bad))) == INV and b"band" in L.sdm_last_error()
    for bad in (dict(clearance=256), dict(max_step=65536)):
        assert L.sdm_world_ground_update(h, vp(opts(**bad))) == INV and b"clearance" in L.sdm_last_error()
    for bad in (0, 17, 0xFFFFFFFF):
        assert L.sdm_world_ground_update(h, vp(opts(radius=bad))) == INV and b"radius" in L.sdm_last_error()
    # the widest band, the largest options; without the flag the box is not read
    assert L.sdm_world_ground_update(h, vp(opts(h_lo=-5, h_hi=4090, clearance=255, max_step=65535, radius=16, tmin=(5, 5), tmax=(4, 4)))) == 0
    # the getter
    assert L.sdm_get_world_ground(h, None, None, None, 0, 0, C.byref(k64), vp(info)) == 0 and k64.value == 1 and info["options"]["radius"][0] == 16
    assert L.sdm_get_world_ground(h, None, None, None, -1, 0, C.byref(k64), None) == INV
    assert L.sdm_get_world_ground(h, None, None, None, 0, -1, C.byref(k64), None) == INV
    assert L.sdm_get_world_ground(h, None, None, None, 0, 0, None, None) == INV
    # the queries
    assert L.sdm_query_world_ground(h, None, None, 0, vp(out), 0) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_query_world_ground(h, vp(xyz), vp(cells), 2, vp(out), 0) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_query_world_ground(h, vp(xyz), None, -1, vp(out), 0) == INV and L.sdm_query_world_ground(h, vp(xyz), None, 2, None, 0) == INV
    assert L.sdm_query_world_ground(h, vp(xyz), None, 2, vp(out), 0x80) == INV
    assert L.sdm_query_world_ground(h, vp(xyz), None, 2, vp(out), 0) == 0
    assert L.sdm_query_world_footprints(h, None, 2, vp(fout), 0) == INV and L.sdm_query_world_footprints(h, vp(fps), 2, None, 0) == INV
    assert L.sdm_query_world_footprints(h, vp(fps), -1, vp(fout), 0) == INV and L.sdm_query_world_footprints(h, vp(fps), 2, vp(fout), 0x80) == INV
    assert L.sdm_query_world_footprints(h, vp(fps), 2, vp(fout), 0) == 0
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert L.sdm_world_ground_update(shard.h, vp(opts())) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_get_world_ground(shard.h, None, None, None, 0, 0, C.byref(k64), None) == INV
    assert L.sdm_query_world_ground(shard.h, vp(xyz), None, 2, vp(out), 0) == INV
    assert L.sdm_query_world_footprints(shard.h, vp(fps), 2, vp(fout), 0) == INV
    shard.close()


# ---- agreement with the block's layer
@pytest.mark.parametrize("up", [(2, 1), (1, -1), (0, 1)])
def test_the_block_archived_once_gives_the_blocks_own_ground_layer(up):
    cfg = gc.block_config()
    N, R = 32, gc.BLOCK_RADIUS
    occ, label, track = gc.block_scene(up)
    ring = sc.crafted_ring(cfg, [0, 0, 0])
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    g.load_state(sc.crafted_state(cfg, ring, _cells(occ == 1), _cells(occ == -1), tracks=track[occ == 1], labels=label[occ == 1]))
    g.set_ring_state(ring)
    depth = np.full((cfg["height"], cfg["width"]), np.nan, np.float32)
    g.update(depth, np.zeros(cfg["height"] * cfg["width"], synth.LABELED_POINT), np.array(ring["last_pos"], np.float32),
             synth.yaw_quat(0.0).astype(np.float32), None, sync=True)
    assert g.ring_state()["moved_steps"] == [0, 0, 0]
    g.world_update()
    band = gc.BLOCK_BAND
    assert band["h_hi"] + band["clearance"] < N
    for flags in (dict(), dict(unknown_passable=True, ignore_movable=True, none_is_lethal=True)):
        g.ground_update(up=up, support_labels=[synth.LABEL_ROAD], **band, **flags)
        b_cells, b_d2, b_info, _ = g.ground()
        assert (b_cells["level"] != gr.NO_LEVEL).mean() >= 0.25
        # block cell i is world cell i - N / 2 on every axis, so a block height h is the world height h - N / 2 for both signs
        ref = check_build(g, max_movable=cfg["max_movable_track"], up=up, h_lo=band["h_lo"] - N // 2, h_hi=band["h_hi"] - N // 2,
                          clearance=band["clearance"], max_step=band["max_step"], radius=R, support_labels=[synth.LABEL_ROAD], **flags)
        coords, w_cells, w_d2, w_info = g.world_ground()
        assert len(coords) == 16 and coords.min() == -2 and coords.max() == 1
        # the tiles as one grid [j_v, i_u] of the block's columns
        grid = np.zeros((N, N), binding.GROUND_CELL)
        d2 = np.zeros((N, N), np.uint16)
        for r, (bu, bv) in enumerate(coords.astype(np.int64).tolist()):
            sl = (slice(8 * bv + 16, 8 * bv + 24), slice(8 * bu + 16, 8 * bu + 24))
            grid[sl], d2[sl] = w_cells[r].reshape(8, 8), w_d2[r].reshape(8, 8)
        has = b_cells["level"] != gr.NO_LEVEL
        assert np.array_equal(grid["level"] != gr.NO_LEVEL, has)
        assert np.array_equal(grid["level"][has].astype(np.int64) + band["h_lo"], b_cells["level"][has])
        seen = b_cells["top"] != gr.NO_LEVEL
        assert np.array_equal(grid["top"] != gr.NO_LEVEL, seen) and np.array_equal(grid["top"][seen].astype(np.int64) + band["h_lo"], b_cells["top"][seen])
        for f in ("label", "n_unknown", "cls"):
            assert np.array_equal(grid[f], b_cells[f]), f
        for k in ("n_ground", "n_obstacle", "n_none", "n_step", "n_lethal"):
            assert int(w_info[k]) == int(b_info[k]), k
        inner = (slice(R, N - R), slice(R, N - R))
        near = b_d2[inner] <= R * R
        assert near.any()
        assert np.array_equal(d2[inner][near], b_d2[inner][near]) and (d2[inner][~near] == NONE).all()
    g.close()
