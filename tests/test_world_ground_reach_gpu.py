"""sdm_world_ground_reach_update / sdm_get_world_ground_reach / sdm_query_world_ground_reach / sdm_world_ground_reach_paths
(include/sdm.h) against tests/world_ground_reach_ref.py's SparseReach, bit for bit: coords, costs, info without `rounds`,
query results and paths.  The model is fed with what world_ground() of the same map returns.

The archive needs a map only as a handle: every case but the last feeds the hand-written bricks of
tests/world_ground_reach_cases.py to world_import on a fresh map of shape A (4 cells an axis)."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import test_world_gpu as twg
from tests import world_ground_reach_cases as rc
from tests import world_ground_reach_ref as ref
from tests.test_ground_gpu import _cells
from tests.test_world_ground_gpu import unusable_entries

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV = 1
CFG = rc.CFG
SIZE = rc.SIZE
FILL = rc.FILL
NO = rc.NO
CASES = rc.crafted()
CAN = 0xA5


def handle():
    return binding.SdmMap(CFG, PARAMS, synth.noise_table())


def world_of(c):
    g = handle()
    g.world_import(c["hdr"], c["cells"])
    return g


def centres(cells, size=SIZE):
    return ((np.asarray(cells, np.int64).astype(np.float32) + np.float32(0.5)) * np.float32(size)).astype(np.float32)


def model_of(g, starts, **kw):
    """the restatement, fed with the ground layer the map itself returns"""
    coords, cells, d2, info = g.world_ground()
    return ref.SparseReach(coords, cells, d2, info["options"], starts, stamp=int(info["stamp"]), **kw)


def check_build(g, starts, size=SIZE, **kw):
    """one build on the map and in the restatement"""
    m = model_of(g, starts, **kw)
    g.world_ground_reach_update(start_cells=np.asarray(starts, np.int32).reshape(-1, 3), **kw)
    got = g.world_ground_reach()
    diff = ref.difference(got, ref.answer(m))
    assert diff is None, diff
    n = len(m.coords)
    print("tiles", n, "rounds", int(got[2]["rounds"]), "tiles relaxed", g.world_ground_reach_tiles_relaxed())
    assert int(got[2]["rounds"]) <= 64 * n + 8 and (n == 0 or got[2]["n_starts_used"] == 0 or got[2]["rounds"] >= 1)
    return m


def check_goals(g, m, goals, size=SIZE, max_len=None):
    goals = np.asarray(goals, np.int32).reshape(-1, 3)
    want = m.query(goals, size)
    got = g.query_world_ground_reach(cells=goals)
    assert got.tobytes() == want.tobytes(), (got[got != want][:3], want[got != want][:3])
    long_rows, long_lens = m.paths(goals, 2000, FILL)
    for k in ([max_len] if max_len is not None else [int(long_lens.max()) if len(goals) else 0, 3]):
        rows, lens = g.world_ground_reach_paths(cells=goals, max_len=k)
        want_rows, want_lens = m.paths(goals, k, FILL)
        assert np.array_equal(lens, want_lens) and np.array_equal(lens, long_lens) and np.array_equal(rows, want_rows)
    return want


def layer_bytes(g, goals):
    coords, cost, info = g.world_ground_reach()
    rows, lens = g.world_ground_reach_paths(cells=goals, max_len=40)
    return [coords.tobytes(), cost.tobytes(), ref.info_without_rounds(info).tobytes(), g.query_world_ground_reach(cells=goals).tobytes(),
            rows.tobytes(), lens.tobytes()]


# ---- the crafted cases
@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_archives(name):
    c = CASES[name]
    g = world_of(c)
    g.world_ground_update(**c["gkw"])
    m = check_build(g, c["starts"], **c["kw"])
    c["expect"](m)                    # (the library's answer is the model's, bit for bit)
    check_goals(g, m, rc.sample_goals(m, c["up"], 8, seed=len(name)))
    g.close()


# ---- the random archive: three orientations x two ground flag sets, each under every reach option
def test_the_random_archive_under_every_option():
    hdr, cells = rc.random_world()
    g = world_of(dict(hdr=hdr, cells=cells))
    builds = 0
    for k, gkw in enumerate(rc.RANDOM_GROUNDS):
        g.world_ground_update(**gkw)
        coords, gcells, d2, info = g.world_ground()
        starts = rc.random_starts(type("G", (), dict(o=info["options"], coords=coords, cells=gcells))())
        assert len(starts) == 32
        for kw in rc.random_reaches():
            m = check_build(g, starts, **kw)
            check_goals(g, m, rc.sample_goals(m, gkw["up"], 4, seed=k), max_len=9)
            builds += 1
    assert builds == 6 * 16
    g.close()


# ---- queries and paths: points and cells, host and device mode, canaries, n = 0, a max_len shorter than the path
def test_queries_and_paths_in_host_and_device_mode():
    c = CASES["penalty 5"]
    g = world_of(c)
    g.world_ground_update(**c["gkw"])
    m = check_build(g, c["starts"], **c["kw"])
    special = np.array([(262143, 0, 0), (262144, 0, 0), (0, -262145, 0), (1 << 30, 0, 0), (0, 0, -(1 << 31)), (3, 2, 1 << 20)], np.int64)
    goals = np.concatenate([special, rc.sample_goals(m, c["up"], 12, seed=3), [rc.cell(c["up"], 7, 1), rc.cell(c["up"], 7, 3, -7), rc.cell(c["up"], 0, 1)]]).astype(np.int32)
    n = len(goals)
    want = m.query(goals, SIZE)
    assert set(want["status"].tolist()) == {0, 2, 3} and (want["next"] == 4).any() and (want["cost"] == 86).any()
    host = g.query_world_ground_reach(cells=goals)
    assert host.tobytes() == want.tobytes()
    # by points: the centres of the cells a float32 holds, and a NaN, an infinity and two points beyond the brick range
    ok = (np.abs(goals.astype(np.int64)) < (1 << 18)).all(axis=1)
    bad = np.array([(np.nan, 0, 0), (0, np.inf, 0), (3e9, 0, 0), (0, 0, -3e9)], np.float32)
    pts = np.concatenate([centres(goals[ok]), bad])
    want_p = np.concatenate([want[ok], m.query([(1 << 30, 0, 0)] * len(bad), SIZE)])
    host_p = g.query_world_ground_reach(xyz=pts)
    assert host_p.tobytes() == want_p.tobytes()
    full_rows, full_lens = m.paths(goals, 64, FILL)
    longest = int(full_lens.max())
    assert longest == 8
    for max_len in (longest, 3, 0):
        for src, expect, kw in ((goals, host, "cells"), (pts, host_p, "xyz")):
            k = len(src)
            cells_like = goals if kw == "cells" else np.concatenate([goals[ok], np.full((len(bad), 3), 1 << 30)])
            want_rows, want_lens = m.paths(cells_like, max_len, FILL)
            rows_h, lens_h = g.world_ground_reach_paths(**{kw: src}, max_len=max_len)
            assert np.array_equal(lens_h, want_lens) and np.array_equal(rows_h, want_rows)     # the rest of a row is left untouched
            d_in = g.device_put(src)
            d_out = g.device_put(np.full(k * 24 + 16, CAN, np.uint8))      # 8 bytes of canary before and behind
            d_rows = g.device_put(np.full(k * max_len * 12 + 16, CAN, np.uint8))
            d_lens = g.device_put(np.full(k * 4 + 16, CAN, np.uint8))
            g.query_world_ground_reach(**{kw: d_in}, on_device=True, n=k, out=d_out + 8)
            g.world_ground_reach_paths(**{kw: d_in}, max_len=max_len, on_device=True, n=k, cells_out=d_rows + 8, len_out=d_lens + 8)
            g.synchronize()
            out = g.device_download(d_out, k * 24 + 16)
            assert (out[:8] == CAN).all() and (out[-8:] == CAN).all() and out[8:-8].tobytes() == expect.tobytes()
            lens = g.device_download(d_lens, k * 4 + 16)
            assert (lens[:8] == CAN).all() and (lens[-8:] == CAN).all() and lens[8:-8].tobytes() == want_lens.tobytes()
            rows = g.device_download(d_rows, k * max_len * 12 + 16)
            assert (rows[:8] == CAN).all() and (rows[-8:] == CAN).all()
            rows = rows[8:-8].view(np.int32).reshape(k, max_len, 3)
            for row, w_row, ln in zip(rows, want_rows, want_lens):
                t = min(int(ln), max_len)
                assert np.array_equal(row[:t], w_row[:t]) and (row[t:].view(np.uint8) == CAN).all()
            for p in (d_in, d_out, d_rows, d_lens):
                g.device_free(p)
    # host mode writes nothing behind its n results; n == 0 is fine
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full((n + 1) * 24, CAN, np.uint8)
    assert L.sdm_query_world_ground_reach(h, None, vp(goals), n, vp(out), 0) == 0
    assert (out[n * 24:] == CAN).all() and out[:n * 24].tobytes() == host.tobytes()
    out[:] = CAN
    lens = np.full(4, 0x5A5A5A5A, np.int32)
    assert L.sdm_query_world_ground_reach(h, None, vp(goals), 0, vp(out), 0) == 0 and (out == CAN).all()
    assert L.sdm_world_ground_reach_paths(h, None, vp(goals), 0, 5, vp(out), vp(lens), 0) == 0 and (out == CAN).all() and (lens == 0x5A5A5A5A).all()
    assert L.sdm_world_ground_reach_paths(h, vp(pts), None, 2, 0, None, vp(lens), 0) == 0 and (lens[2:] == 0x5A5A5A5A).all()
    g.close()


# ---- entries that stand for no world cell: as starts they count for nothing, as goals nothing of them reaches the result
def test_entries_that_stand_for_no_world_cell():
    c = CASES["penalty 5"]
    g = world_of(c)
    g.world_ground_update(**c["gkw"])
    pts, cells = unusable_entries(SIZE)
    starts = np.asarray(c["starts"], np.int32).reshape(-1, 3)
    m = check_build(g, np.concatenate([starts, cells]), **c["kw"])      # (by cells)
    assert m.info["n_starts_used"] == len(set(map(tuple, starts.tolist()))) > 0
    g.world_ground_reach_update(starts=np.concatenate([centres(starts), pts]), **c["kw"])
    diff = ref.difference(g.world_ground_reach(), ref.answer(m))
    assert diff is None, diff
    none = m.query([(1 << 30, 0, 0)], SIZE)
    assert none["status"][0] == 3
    want_c, want_p = m.query(cells, SIZE), np.repeat(none, len(pts))
    assert want_c.tobytes() == np.repeat(none, len(cells)).tobytes()
    assert g.query_world_ground_reach(cells=cells).tobytes() == want_c.tobytes()
    assert g.query_world_ground_reach(xyz=pts).tobytes() == want_p.tobytes()
    for kw, src in (("cells", cells), ("xyz", pts)):
        rows, lens = g.world_ground_reach_paths(**{kw: src}, max_len=4)
        assert not lens.any() and (rows == FILL).all()
    g.close()


# ---- the ranges of the getter
def test_getter_ranges_and_canaries():
    c = CASES["serpentine"]
    g = world_of(c)
    g.world_ground_update(**c["gkw"])
    m = check_build(g, c["starts"], **c["kw"])
    n = len(m.coords)
    assert n == 9
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = C.c_int64(-1)
    for first, cap in ((0, n), (3, 4), (n - 2, 6), (n, 4), (n + 5, 4), (2, 0)):
        take = max(min(n - first, cap), 0)
        cb, wb = np.full((cap + 2, 2), 0x5A5A, np.int16), np.full((cap + 2, 64), 0xA5A5A5A5, np.uint32)
        assert L.sdm_get_world_ground_reach(h, vp(cb), vp(wb), first, cap, C.byref(got), None) == 0 and got.value == n
        assert np.array_equal(cb[:take], m.coords[first:first + take]) and (cb[take:] == 0x5A5A).all()
        assert np.array_equal(wb[:take], m.cost[first:first + take]) and (wb[take:] == 0xA5A5A5A5).all()
    part = g.world_ground_reach(first=4, cap=3)
    assert np.array_equal(part[0], m.coords[4:7]) and np.array_equal(part[1], m.cost[4:7]) and g.world_ground_reach(with_cost=False)[1] is None
    assert np.array_equal(g.world_ground()[0], m.coords)                # without a box: the ground layer's rows
    info = np.zeros(1, binding.WORLD_GROUND_REACH_INFO)
    assert L.sdm_get_world_ground_reach(h, None, None, 0, n, C.byref(got), vp(info)) == 0 and got.value == n
    assert ref.info_without_rounds(info[0]).tobytes() == m.info.tobytes() and info["pad"][0] == 0
    g.close()


# ---- the build is a snapshot
def test_the_build_is_a_snapshot():
    c = CASES["four tiles round a corner, up 1 -1"]
    g = world_of(c)
    g.world_ground_update(**c["gkw"])
    m = check_build(g, c["starts"], **c["kw"])
    goals = rc.sample_goals(m, c["up"], 10, seed=5).astype(np.int32)
    before = layer_bytes(g, goals)
    assert before[3] == m.query(goals, SIZE).tobytes()
    g.world_ground_update(**dict(c["gkw"], up=(2, 1), h_lo=-3, h_hi=2, radius=2))     # another band, another up axis
    assert layer_bytes(g, goals) == before
    other = CASES["seam in u"]
    g.world_import(other["hdr"], other["cells"], offset=(3, 0, -5))
    assert layer_bytes(g, goals) == before
    assert g.world_retain(bmin=(100, 100, 100), bmax=(101, 101, 101)) > 0 and g.world_info()["n_bricks"] == 0       # the archive is empty
    assert layer_bytes(g, goals) == before
    g.world_clear()
    assert layer_bytes(g, goals) == before
    g.world_import(c["hdr"], c["cells"])
    g.world_ground_update(**c["gkw"])
    assert layer_bytes(g, goals) == before                              # (and a new ground build of the same archive changes nothing either)
    g.close()


# ---- two runs; a smaller build after a larger one; a larger one again
def test_two_runs_and_a_smaller_build_after_a_larger_one():
    big, small = CASES["serpentine"], CASES["budget"]
    g = world_of(big)
    g.world_ground_update(**big["gkw"])
    state = lambda: [a.tobytes() for a in g.world_bricks()] + [np.asarray(a).tobytes() for a in g.world_ground()] + [g.world_info().tobytes()]  # noqa: E731
    before = state()
    goals = rc.sample_goals(model_of(g, big["starts"], **big["kw"]), big["up"], 10, seed=1).astype(np.int32)
    runs = []
    for _ in range(2):
        m = check_build(g, big["starts"], **big["kw"])
        runs.append(layer_bytes(g, goals))
    assert runs[0] == runs[1] and state() == before                     # nothing of the ground layer or the archive is modified
    g.world_clear()
    g.world_import(small["hdr"], small["cells"])
    g.world_ground_update(**small["gkw"])
    m = check_build(g, small["starts"], **small["kw"])
    small["expect"](m)
    assert g.query_world_ground_reach(cells=[rc.cell((2, 1), 12, 12)])["status"][0] == 3     # a tile of the larger build's table
    g.world_clear()
    g.world_import(big["hdr"], big["cells"])
    g.world_ground_update(**big["gkw"])
    check_build(g, big["starts"], **big["kw"])
    assert layer_bytes(g, goals) == runs[0]
    g.close()


# ---- the argument checks
def test_argument_errors():
    g = handle()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    info = np.zeros(1, binding.WORLD_GROUND_REACH_INFO)

    def opts(**kw):
        o = np.zeros(1, binding.WORLD_GROUND_REACH_OPTIONS)
        for k, v in kw.items():
            o[k] = v
        return o

    out = np.zeros(2, binding.WORLD_GROUND_REACH_RESULT)
    cells, xyz = np.zeros((2, 3), np.int32), np.zeros((2, 3), np.float32)
    rows, lens = np.zeros((2, 4, 3), np.int32), np.zeros(2, np.int32)
    k64 = C.c_int64(-7)
    c = CASES["clearance min_d2 0"]                                      # R = 3
    g.world_import(c["hdr"], c["cells"])
    # before any ground build; the getter and the queries before any build
    assert L.sdm_world_ground_reach_update(h, vp(opts()), None, vp(cells), 2) == INV and b"sdm_world_ground_update first" in L.sdm_last_error()
    g.world_ground_update(**c["gkw"])
    assert L.sdm_get_world_ground_reach(h, None, None, 0, 0, C.byref(k64), vp(info)) == INV and b"sdm_world_ground_reach_update first" in L.sdm_last_error()
    assert L.sdm_query_world_ground_reach(h, None, vp(cells), 2, vp(out), 0) == INV and b"sdm_world_ground_reach_update first" in L.sdm_last_error()
    assert L.sdm_world_ground_reach_paths(h, None, vp(cells), 2, 4, vp(rows), vp(lens), 0) == INV and b"sdm_world_ground_reach_update first" in L.sdm_last_error()
    assert k64.value == -7
    # the build's arguments
    assert L.sdm_world_ground_reach_update(None, vp(opts()), None, vp(cells), 2) == INV
    assert L.sdm_world_ground_reach_update(h, None, None, vp(cells), 2) == INV
    assert L.sdm_world_ground_reach_update(h, vp(opts(flags=4)), None, vp(cells), 2) == INV and b"flag" in L.sdm_last_error()
    for bad in (dict(pad=(1, 0)), dict(pad=(0, 7))):
        assert L.sdm_world_ground_reach_update(h, vp(opts(**bad)), None, vp(cells), 2) == INV and b"pad" in L.sdm_last_error()
    for bad in (dict(penalty=65536), dict(max_climb=65536), dict(penalty=0xFFFFFFFF)):
        assert L.sdm_world_ground_reach_update(h, vp(opts(**bad)), None, vp(cells), 2) == INV and b"65535" in L.sdm_last_error()
    for bad in (dict(min_d2=11), dict(soft_d2=11), dict(min_d2=0xFFFFFFFF)):      # R^2 + 2
        assert L.sdm_world_ground_reach_update(h, vp(opts(**bad)), None, vp(cells), 2) == INV and b"R^2 + 1" in L.sdm_last_error()
    assert L.sdm_world_ground_reach_update(h, vp(opts()), None, None, 0) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_world_ground_reach_update(h, vp(opts()), vp(xyz), vp(cells), 2) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_world_ground_reach_update(h, vp(opts()), vp(xyz), None, -1) == INV
    assert L.sdm_get_world_ground_reach(h, None, None, 0, 0, C.byref(k64), None) == INV           # (a refused build is no build)
    # the largest options; without the flag the box is not read; a count of 0 with one pointer
    assert L.sdm_world_ground_reach_update(h, vp(opts(min_d2=10, soft_d2=10, penalty=65535, max_climb=65535, max_cost=0xFFFFFFFF, tmin=(5, 5),
                                                      tmax=(4, 4))), vp(xyz), None, 0) == 0
    assert L.sdm_get_world_ground_reach(h, None, None, 0, 0, C.byref(k64), vp(info)) == 0 and k64.value == 1 and info["options"]["penalty"][0] == 65535
    assert info["n_starts_used"][0] == 0 and info["n_reached"][0] == 0 and info["n_traversable"][0] == 7
    # the getter
    assert L.sdm_get_world_ground_reach(h, None, None, -1, 0, C.byref(k64), None) == INV
    assert L.sdm_get_world_ground_reach(h, None, None, 0, -1, C.byref(k64), None) == INV
    assert L.sdm_get_world_ground_reach(h, None, None, 0, 0, None, None) == INV
    # the queries
    assert L.sdm_query_world_ground_reach(h, None, None, 0, vp(out), 0) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_query_world_ground_reach(h, vp(xyz), vp(cells), 2, vp(out), 0) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_query_world_ground_reach(h, vp(xyz), None, -1, vp(out), 0) == INV and L.sdm_query_world_ground_reach(h, vp(xyz), None, 2, None, 0) == INV
    assert L.sdm_query_world_ground_reach(h, vp(xyz), None, 2, vp(out), 0x80) == INV
    assert L.sdm_query_world_ground_reach(h, vp(xyz), None, 2, vp(out), 0) == 0
    assert L.sdm_world_ground_reach_paths(h, None, None, 2, 4, vp(rows), vp(lens), 0) == INV and b"exactly one" in L.sdm_last_error()
    assert L.sdm_world_ground_reach_paths(h, vp(xyz), None, 2, -1, vp(rows), vp(lens), 0) == INV
    assert L.sdm_world_ground_reach_paths(h, vp(xyz), None, 2, 4, None, vp(lens), 0) == INV
    assert L.sdm_world_ground_reach_paths(h, vp(xyz), None, 2, 4, vp(rows), None, 0) == INV
    assert L.sdm_world_ground_reach_paths(h, vp(xyz), None, -1, 4, vp(rows), vp(lens), 0) == INV
    assert L.sdm_world_ground_reach_paths(h, vp(xyz), None, 2, 4, vp(rows), vp(lens), 0x80) == INV
    assert L.sdm_world_ground_reach_paths(h, vp(xyz), None, 2, 4, vp(rows), vp(lens), 0) == 0
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert L.sdm_world_ground_reach_update(shard.h, vp(opts()), None, vp(cells), 2) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_get_world_ground_reach(shard.h, None, None, 0, 0, C.byref(k64), None) == INV
    assert L.sdm_query_world_ground_reach(shard.h, vp(xyz), None, 2, vp(out), 0) == INV
    assert L.sdm_world_ground_reach_paths(shard.h, vp(xyz), None, 2, 4, vp(rows), vp(lens), 0) == INV
    shard.close()


# ---- frames, world_update, the ground layer, the frontiers: a route on the ground to a frontier the block has left
def test_a_route_on_the_ground_to_a_world_frontier():
    cfg = sc.config("B")
    N, size = twg.dims(cfg), np.float32(cfg["voxel_size"])
    assert tuple(N) == (4, 32, 64)
    occ = np.zeros(tuple(N[::-1]), np.int8)                             # [z, y, x]: x is up; the floor is the layer x = 0
    occ[:, :, 0] = 1
    occ[10:14, 6:10, 1:] = -1                                           # a pocket nobody has seen, standing on the floor
    occ[30:34, 20:26, 1:] = -1
    occ[20, 12:20, 1] = 1                                               # a low wall
    steps = np.array(sc.crafted_steps(cfg), np.int64)
    ring = sc.crafted_ring(cfg, steps)
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    n_occ = int((occ == 1).sum())
    g.load_state(sc.crafted_state(cfg, ring, _cells(occ == 1), _cells(occ == -1), tracks=np.full(n_occ, 65535), labels=np.full(n_occ, 8)))
    g.set_ring_state(ring)
    twg.blind_frame(g, cfg, ring["last_pos"])
    g.world_update()
    drive = int(N[2]) // 4
    for _ in range(2):                                                  # the camera drives off along z; what comes in is unobserved
        steps[2] += drive // 2
        twg.blind_frame(g, cfg, twg.cam_of(cfg, steps))
        g.world_update()
    up = (0, 1)
    x0 = int(steps[0]) - int(N[0]) // 2                                 # world x of the block's layer x = 0
    g.world_ground_update(up=up, h_lo=x0, h_hi=x0 + 2, clearance=1, max_step=1, radius=4, support_labels=[8])
    g.world_frontiers_update(inside_bricks=True)                         # the pockets' frontiers, not the archive's rim
    clusters, finfo = g.world_frontiers()
    fcells = g.world_frontier_cells()[0]
    assert len(clusters) >= 1 and len(fcells) >= 64
    start = [x0 + 1, int(steps[1]) - 2, int(steps[2]) - drive - 3]      # a cell over the floor the block has partly left
    kw = dict(min_d2=0, soft_d2=5, penalty=7, max_climb=1)
    m = check_build(g, [start], size=size, **kw)
    assert m.info["n_starts_used"] == 1 and m.info["n_reached"] > 500
    # a cluster's first_cell as it is - only the column counts - and frontier cells from all over the list
    goals = np.concatenate([clusters["first_cell"], fcells[::max(len(fcells) // 16, 1)]]).astype(np.int32)
    res = check_goals(g, m, goals, size=size, max_len=400)
    reached = np.flatnonzero(res["status"] == 0)
    assert res["status"][0] == 0 and len(reached) >= 4 and res["cost"][reached].max() >= 200
    rows, lens = g.world_ground_reach_paths(cells=goals, max_len=400)
    for i in reached.tolist():
        cells = rows[i, :lens[i]]
        q = g.query_world_ground(cells=cells)
        assert (q["status"] == 0).all() and ((q["cell"]["cls"] & 3) == 1).all() and ((q["cell"]["cls"] & 8) == 0).all() and (q["above"] == 1).all()
        assert rc.path_sum(m, up, cells.tolist()) == int(res["cost"][i]) and (cells[-1] == start).all()
        for p, q_ in zip(cells[:-1].tolist(), cells[1:].tolist()):      # every step of the way back is an allowed move
            assert m.may((q_[1], q_[2]), p[1] - q_[1], p[2] - q_[2])
    g.close()
