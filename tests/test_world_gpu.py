"""The world archive (include/sdm.h: sdm_world_update / sdm_get_world_info / sdm_get_world_bricks / sdm_get_world_occupied /
sdm_query_world_points / sdm_get_world_region / sdm_world_clear) against tests/world_ref.py, bit for bit: the restatement
is fed the GPU's own voxels() and ring_state() per update, and headers, cells, info, the occupied list and world_region
over the bricks' bounding box plus one brick of margin must be its bytes.

Crafted maps on the shapes of tests/shape_cases.py with the ring at several offsets and the block's min corner at brick
offsets 0, 1 and 7, under every flag combination; a camera that leaves what it has archived; a free-running drive; the
capacity rule; the queries in host and device mode; run-to-run identity; no side effects; the argument checks."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import esdf_ref as er
from tests import query_ref as qr
from tests import shape_cases as sc
from tests import world_ref as wr
from tests.test_ground_gpu import _cells, random_block

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV = 1


def dims(cfg):
    return np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.int64)


def cam_of(cfg, steps):
    """the camera in the middle of the cell the ring follows at `steps` (shape_cases.crafted_ring's rule)"""
    size = np.float32(cfg["voxel_size"])
    return np.array([np.float32(s + (0.5 if s >= 0 else -0.5)) * size for s in steps], np.float32)


def blind_frame(g, cfg, pos):
    """a frame that sees nothing, the camera at pos"""
    depth = np.full((cfg["height"], cfg["width"]), np.nan, np.float32)
    cloud = np.zeros(cfg["height"] * cfg["width"], synth.LABELED_POINT)
    g.update(depth, cloud, np.asarray(pos, np.float32), synth.yaw_quat(0.0).astype(np.float32), None, sync=True)


def crafted(cfg, steps, seed):
    """a map whose result array reads random_block(cfg, seed) on a ring moved by `steps` (test_ground_gpu.crafted_map with
    the ring of the caller's choice)"""
    occ, label, track = random_block(cfg, seed)
    ring = sc.crafted_ring(cfg, steps)
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    g.load_state(sc.crafted_state(cfg, ring, _cells(occ == 1), _cells(occ == -1), tracks=track[occ == 1], labels=label[occ == 1]))
    g.set_ring_state(ring)
    blind_frame(g, cfg, ring["last_pos"])
    assert g.ring_state()["moved_steps"] == [int(s) for s in steps]
    return g


def snapshot(g, cfg):
    ring = g.ring_state()
    return ring, er.snapshot_grid(qr.Geometry(cfg, ring), g.voxels())


def update(g, A, cfg, flags=0, max_bricks=0):
    """one world_update on the map and on the restatement, which reads the map's own results"""
    g.world_update(static_only=bool(flags & wr.STATIC_ONLY), observed_only=bool(flags & wr.OBSERVED_ONLY), max_bricks=max_bricks)
    ring, snap = snapshot(g, cfg)
    wr.merge(A, snap, ring["moved_steps"], ring["global_time_stamp"], cfg["max_movable_track"], flags)
    return ring, snap


def compare(g, A, cfg, tag=""):
    """headers, cells, info, the occupied list and the region around the bricks, bit for bit"""
    info, want_info = g.world_info(), A.info()
    for name in binding.WORLD_INFO.names:
        assert np.array_equal(info[name], want_info[name]), (tag, name, info, want_info)
    assert info.tobytes() == want_info.tobytes()
    hdr, cells = g.world_bricks()
    want_hdr, want_cells = A.bricks()
    assert len(hdr) == len(want_hdr), (tag, len(hdr), len(want_hdr))
    for name in binding.WORLD_BRICK.names:
        bad = np.nonzero(hdr[name] != want_hdr[name])[0]
        assert not len(bad), (tag, name, len(bad), hdr[bad[:3]], want_hdr[bad[:3]])
    assert hdr.tobytes() == want_hdr.tobytes()
    bad = np.argwhere(cells != want_cells)
    assert not len(bad), (tag, "cells", len(bad), bad[:4].tolist())
    pts, n = g.world_occupied()
    want_pts = A.occupied(cfg["voxel_size"])
    assert n == len(want_pts) == int(info["n_occupied"]) and pts.tobytes() == want_pts.tobytes(), (tag, n, len(want_pts))
    if len(hdr):
        lo = info["bmin"].astype(np.int64) * 8 - 8
        size = (info["bmax"].astype(np.int64) - info["bmin"] + 3) * 8
        got = g.world_region(lo, size)
        assert got.shape == tuple(size[::-1]) and np.array_equal(got, A.region(lo, size)), (tag, "region")
    return info


def fresh_archive(cfg, max_bricks=0):
    return wr.Archive(max_bricks or wr.default_max_bricks(dims(cfg)))


def offset_steps(cfg, off, sign):
    """ring offsets that put the block's min corner at brick offset `off` on every axis, a few bricks from the origin"""
    N = dims(cfg)
    return [int(sign * 8 * (3 + a) + off + (N[a] >> 1)) if sign > 0 else int(-8 * (2 + a) + off + (N[a] >> 1)) for a in range(3)]


# ---- crafted maps
STEP_SETS = {
    "A": ["turns", (0, 1), (1, -1), (7, 1)],
    "B": ["turns", (0, -1), (1, 1), (7, -1)],
    "C": ["turns", (0, 1), (1, -1), (7, 1)],
    "D": ["turns", (7, -1)],
    "E": ["turns"],
}


@pytest.mark.parametrize("name", sc.PARITY_CASES)
def test_crafted_maps_under_every_flag_combination(name):
    cfg = sc.config(name)
    for k, spec in enumerate(STEP_SETS[name]):
        steps = sc.crafted_steps(cfg) if spec == "turns" else offset_steps(cfg, *spec)
        if spec != "turns":
            g0 = np.array(steps) - (dims(cfg) >> 1)
            assert ((g0 & 7) == spec[0]).all()
        g = crafted(cfg, steps, seed=40 + k)
        for flags in (wr.ALL_FLAGS if name != "E" else [0, wr.STATIC_ONLY | wr.OBSERVED_ONLY]):
            g.world_clear()
            A = fresh_archive(cfg)
            _, snap = update(g, A, cfg, flags)
            info = compare(g, A, cfg, (name, spec, flags))
            assert info["n_bricks"] == info["created_last"] > 0 and info["dropped_last"] == 0
            if flags & wr.STATIC_ONLY:          # the flag left something out, the archive holds fewer obstacles than the block
                assert info["n_occupied"] < int((wr.occ_of(snap) >= 1).sum())
            # a second update of the same frame changes nothing but the update count
            hdr, cells = g.world_bricks()
            update(g, A, cfg, flags)
            info2 = compare(g, A, cfg, (name, spec, flags, "again"))
            hdr2, cells2 = g.world_bricks()
            assert info2["created_last"] == 0 and hdr2.tobytes() == hdr.tobytes() and cells2.tobytes() == cells.tobytes()
        g.close()


def test_a_brick_beyond_the_coordinate_range_is_never_created():
    cfg = sc.config("A")                              # 4 cells per axis, voxels of 1 m: the block straddles brick 32767 | 32768 on x
    steps = [262143, -262141, 9]                      # x: cells 262141 .. 262144; y: cells -262143 .. -262140, inside the range
    g = crafted(cfg, steps, seed=3)
    A = fresh_archive(cfg)
    update(g, A, cfg)
    info = compare(g, A, cfg, "range")
    assert info["out_of_range_last"] > 0 and info["n_bricks"] > 0 and info["bmax"][0] == 32767 and info["bmin"][1] == -32768
    res = g.query_world(np.array([[262144.5, -262140.5, 9.5], [262143.5, -262140.5, 9.5]], np.float32))
    assert res.tobytes() == A.query_points([[262144.5, -262140.5, 9.5], [262143.5, -262140.5, 9.5]], cfg["voxel_size"]).tobytes()
    assert tuple(res[0]) == (0, 0, -1, 0)
    g.close()


# ---- leaving the block
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_archive_remembers_what_the_block_has_left(name):
    cfg = sc.config(name)
    N = dims(cfg)
    size = np.float32(cfg["voxel_size"])
    steps = np.array(sc.crafted_steps(cfg), np.int64)
    g = crafted(cfg, steps, seed=11)
    A = fresh_archive(cfg)
    update(g, A, cfg)
    compare(g, A, cfg, (name, "start"))
    outside = remembered = moves = 0
    for a in range(3):
        for k in sorted({1, 3, int(N[a]) // 4}):
            for d in (k, -k, -k, k):                   # there and back on both sides: the slab that comes back reads unknown
                steps[a] += d
                blind_frame(g, cfg, cam_of(cfg, steps))
                ring, snap = update(g, A, cfg)
                assert ring["moved_steps"] == steps.tolist()
                moves += 1
                g0 = wr.block_origin(snap, ring["moved_steps"])
                pts, _ = g.world_occupied()
                cell = np.stack([np.floor(pts[c] / size + 0.5) for c in "xyz"], 1).astype(np.int64) - g0   # (min corners: exact multiples)
                outside += int(((cell < 0) | (cell >= N)).any(axis=1).sum())
                z, y, x = np.nonzero(wr.occ_of(snap) == -1)
                if len(x):
                    centre = ((np.stack([x, y, z], 1) + g0).astype(np.float32) + np.float32(0.5)) * size
                    got = g.query_world(centre)
                    assert got.tobytes() == A.query_points(centre, cfg["voxel_size"]).tobytes()
                    remembered += int((got["occ"] >= 0).sum())
        compare(g, A, cfg, (name, "axis", a))
    assert outside > 0 and remembered > 0, (name, moves, outside, remembered)
    g.close()


# ---- a free-running drive
@pytest.mark.parametrize("name", ["B", "C"])
def test_a_free_running_drive(name):
    cfg = sc.config(name)
    n_frames = 20
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    A = fresh_archive(cfg)
    at = set(np.linspace(0, n_frames - 1, 5).astype(int).tolist())
    for t, depth, cloud, pos, q, mv, remove in sc.drive(name, PARAMS, n_frames, seed=29):
        g.update(depth, cloud, pos, q, mv, remove, sync=True)
        flags = wr.ALL_FLAGS[t % 4]
        update(g, A, cfg, flags)
        if t in at:
            compare(g, A, cfg, (name, "frame", t))
    info = g.world_info()
    assert info["n_updates"] == n_frames and info["n_bricks"] > 0
    blk = (dims(cfg) + 7) // 8 + 1
    assert ((info["bmax"] - info["bmin"] + 1) > blk).any()     # the jump: the archive spans more than any one block
    g.close()


# ---- capacity
def test_capacity_drops_the_highest_ranked_new_bricks():
    cfg = sc.config("B")
    g = crafted(cfg, sc.crafted_steps(cfg), seed=5)
    A = fresh_archive(cfg, 5)
    update(g, A, cfg, 0, max_bricks=5)
    info = compare(g, A, cfg, "capacity 5")
    assert info["n_bricks"] == info["created_last"] == info["max_bricks"] == 5 and info["dropped_last"] > 0
    assert info["dropped_total"] == info["dropped_last"]
    full = fresh_archive(cfg)
    _, snap = snapshot(g, cfg)
    wr.merge(full, snap, g.ring_state()["moved_steps"], 0, cfg["max_movable_track"], 0)
    coords = lambda hdr: np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1)  # noqa: E731
    assert len(full.coord) > 5 and np.array_equal(coords(g.world_bricks()[0]), coords(full.bricks()[0])[:5])   # the first five in brick order
    with pytest.raises(binding.SdmError, match="max_bricks"):
        g.world_update(max_bricks=64)
    update(g, A, cfg, 0, max_bricks=5)                 # the same capacity, and 0, are taken
    update(g, A, cfg, 0, max_bricks=0)
    info = compare(g, A, cfg, "capacity 5 again")
    assert info["n_bricks"] == 5 and info["created_last"] == 0 and info["dropped_total"] == 3 * info["dropped_last"]
    g.world_clear()
    zero = g.world_info()
    assert all(zero[f] == 0 for f in ("n_bricks", "max_bricks", "n_updates", "dropped_total", "n_occupied", "flags", "stamp")) and (zero["bmax"] == -1).all()
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        g.world_bricks()
    A = fresh_archive(cfg, 4096)
    update(g, A, cfg, 0, max_bricks=4096)
    info = compare(g, A, cfg, "fresh capacity")
    assert info["max_bricks"] == 4096 and info["n_bricks"] == len(full.coord) and info["dropped_last"] == 0 and info["dropped_total"] == 0
    g.close()


# ---- queries
def test_queries_in_host_and_device_mode():
    cfg = sc.config("C")
    steps = [-21, 5, -70]                              # negative world coordinates on x and z
    g = crafted(cfg, steps, seed=8)
    A = fresh_archive(cfg)
    ring, snap = update(g, A, cfg, wr.STATIC_ONLY)
    N, size = dims(cfg), np.float32(cfg["voxel_size"])
    g0 = wr.block_origin(snap, ring["moved_steps"])
    assert (g0 < 0).any()
    rng = np.random.default_rng(2)
    cells = np.concatenate([rng.integers(g0 - 20, g0 + N + 20, (4000, 3)), np.stack(np.meshgrid(*(np.arange(n) for n in N), indexing="ij"), -1).reshape(-1, 3) + g0])
    xyz = ((cells.astype(np.float32) + np.float32(0.5)) * size).astype(np.float32)
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [-1e30, 1e30, 0], [3e38, 3e38, 3e38]], np.float32)
    xyz = np.concatenate([xyz, special])
    got = g.query_world(xyz)
    want = A.query_points(xyz, cfg["voxel_size"])
    assert got.tobytes() == want.tobytes()
    assert (got["occ"] >= 0).any() and (got["occ"][:4000] == -1).any() and (got[-len(special):].tobytes() == np.array([(0, 0, -1, 0)] * len(special), binding.WORLD_CELL).tobytes())
    # device mode: identical bytes
    d_xyz, d_out = g.device_put(xyz), g.device_alloc(len(xyz) * 8)
    g.query_world(d_xyz, on_device=True, n=len(xyz), out=d_out)
    g.synchronize()
    assert g.device_download(d_out, len(xyz) * 8).tobytes() == got.tobytes()
    # inside the block the archive says what the map says, wherever the block cell wrote
    inside = xyz[4000:-len(special)]
    now = g.query_points(inside)
    wrote = wr.writes(now.view(np.uint32).reshape(-1, 2)[:, 1], cfg["max_movable_track"], wr.STATIC_ONLY)
    arch = got[4000:-len(special)]
    assert wrote.any() and not wrote.all()
    for f in ("track", "label", "occ"):
        assert np.array_equal(arch[f][wrote], now[f][wrote]), f
    assert (arch["stamp"][wrote] == ring["global_time_stamp"]).all() and (arch["occ"][~wrote] == -1).all()
    # the region, host and device
    lo, sz = g0 - 5, N + 11
    words = g.world_region(lo, sz)
    assert np.array_equal(words, A.region(lo, sz))
    d_words = g.device_alloc(words.size * 4)
    g.world_region(lo, sz, on_device=True, out=d_words)
    g.synchronize()
    assert g.device_download(d_words, words.size * 4).tobytes() == words.tobytes()
    for p in (d_xyz, d_out, d_words):
        g.device_free(p)
    g.close()


def test_canaries_behind_every_caller_buffer():
    cfg = sc.config("B")
    g = crafted(cfg, sc.crafted_steps(cfg), seed=6)
    g.world_update()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hdr, cells = g.world_bricks()
    pts, n_pts = g.world_occupied()
    n = len(hdr)
    assert n > 6 and n_pts > 10
    got = C.c_int64()
    first, cap = 2, n - 5
    b = np.full((cap + 2) * 20, 0xA5, np.uint8)
    c = np.full((cap + 2, 512), 0xA5A5A5A5, np.uint32)
    assert L.sdm_get_world_bricks(h, vp(b), vp(c), first, cap, C.byref(got)) == 0 and got.value == n
    assert b[:cap * 20].tobytes() == hdr[first:first + cap].tobytes() and np.array_equal(c[:cap], cells[first:first + cap])
    assert (b[cap * 20:] == 0xA5).all() and (c[cap:] == 0xA5A5A5A5).all()
    assert L.sdm_get_world_bricks(h, vp(b), vp(c), n + 3, cap, C.byref(got)) == 0 and got.value == n      # first beyond the end: nothing
    assert (b[cap * 20:] == 0xA5).all()
    cap = n_pts - 7
    p = np.full((cap + 3) * 16, 0xA5, np.uint8)
    assert L.sdm_get_world_occupied(h, vp(p), cap, C.byref(got), 0) == 0 and got.value == n_pts
    assert p[:cap * 16].tobytes() == pts[:cap].tobytes() and (p[cap * 16:] == 0xA5).all()
    xyz = np.zeros((5, 3), np.float32)
    out = np.full(8 * 8, 0xA5, np.uint8)
    assert L.sdm_query_world_points(h, vp(xyz), 5, vp(out), 0) == 0 and (out[40:] == 0xA5).all() and not (out[:40] == 0xA5).all()
    lo, sz = np.array([0, 0, 0], np.int32), np.array([3, 5, 2], np.int32)
    w = np.full(30 + 4, 0xA5A5A5A5, np.uint32)
    assert L.sdm_get_world_region(h, vp(lo), vp(sz), vp(w), 0) == 0 and (w[30:] == 0xA5A5A5A5).all() and not (w[:30] == 0xA5A5A5A5).any()
    g.close()


# ---- reproducibility, no side effects
def run_drive(cfg, name, n_frames, archive):
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    out = []
    for t, depth, cloud, pos, q, mv, remove in sc.drive(name, PARAMS, n_frames, seed=31):
        g.update(depth, cloud, pos, q, mv, remove, sync=True)
        if archive:
            g.world_update(static_only=bool(t & 1))
            if t % 3 == 0:
                g.world_occupied()
                g.query_world(np.array([pos], np.float32))
                g.world_region([0, 0, 0], [4, 4, 4])
    if archive:
        info = g.world_info()
        hdr, cells = g.world_bricks()
        lo = info["bmin"].astype(np.int64) * 8
        out = [info.tobytes(), hdr.tobytes(), cells.tobytes(), g.world_occupied()[0].tobytes(),
               g.world_region(lo, (info["bmax"].astype(np.int64) - info["bmin"] + 1) * 8).tobytes()]
    return g, out


def test_two_runs_are_identical_and_the_map_is_left_alone():
    name = "B"
    cfg = sc.config(name)
    g1, out1 = run_drive(cfg, name, 8, True)
    g2, out2 = run_drive(cfg, name, 8, True)
    assert out1 == out2 and len(out1[1]) > 0
    g3, _ = run_drive(cfg, name, 8, False)
    assert g1.voxels().tobytes() == g3.voxels().tobytes()
    s1, s3 = g1.dump_state(), g3.dump_state()
    for k in s1:
        assert s1[k].tobytes() == s3[k].tobytes(), k
    g1.world_clear()
    frames = list(sc.drive(name, PARAMS, 10, seed=31))
    for g in (g1, g3):
        t, depth, cloud, pos, q, mv, remove = frames[9]
        g.update(depth, cloud, pos, q, mv, remove, sync=True)
    assert g1.voxels().tobytes() == g3.voxels().tobytes() and g1.ring_state() == g3.ring_state()
    for g in (g1, g2, g3):
        g.close()


def test_sdm_clear_and_set_ring_state_leave_the_archive_alone():
    cfg = sc.config("A")
    g = crafted(cfg, [9, -3, 20], seed=9)
    A = fresh_archive(cfg)
    update(g, A, cfg)
    ring = g.ring_state()
    g.clear()
    g.set_ring_state(ring)
    compare(g, A, cfg, "after clear")
    g.close()


# ---- the argument checks
def test_argument_errors():
    cfg = sc.config("A")
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o, info = np.zeros(1, binding.WORLD_OPTIONS), np.zeros(1, binding.WORLD_INFO)
    got = C.c_int64(-7)
    xyz, out = np.zeros((2, 3), np.float32), np.zeros(2, binding.WORLD_CELL)
    lo, sz, words = np.zeros(3, np.int32), np.ones(3, np.int32), np.zeros(8, np.uint32)
    # before any update: info answers zeros, everything else is refused
    assert L.sdm_get_world_info(h, vp(info)) == 0 and info["n_bricks"][0] == 0 and (info["bmax"][0] == -1).all()
    assert L.sdm_get_world_bricks(h, None, None, 0, 0, C.byref(got)) == INV and b"sdm_world_update first" in L.sdm_last_error()
    assert L.sdm_get_world_occupied(h, None, 0, C.byref(got), 0) == INV
    assert L.sdm_query_world_points(h, vp(xyz), 2, vp(out), 0) == INV
    assert L.sdm_get_world_region(h, vp(lo), vp(sz), vp(words), 0) == INV and got.value == -7
    assert L.sdm_world_clear(h) == 0
    assert L.sdm_world_update(h, None) == INV and L.sdm_get_world_info(h, None) == INV
    o["flags"] = 4
    assert L.sdm_world_update(h, vp(o)) == INV and b"flag" in L.sdm_last_error()
    o["flags"], o["max_bricks"] = 0, -1
    assert L.sdm_world_update(h, vp(o)) == INV
    o["max_bricks"] = (1 << 21) + 1
    assert L.sdm_world_update(h, vp(o)) == INV
    blind_frame(g, cfg, [0.5, 0.5, 0.5])
    g.world_update()
    assert L.sdm_get_world_bricks(h, None, None, -1, 0, C.byref(got)) == INV and L.sdm_get_world_bricks(h, None, None, 0, -1, C.byref(got)) == INV
    assert L.sdm_get_world_bricks(h, None, None, 0, 0, None) == INV
    assert L.sdm_get_world_occupied(h, None, -1, C.byref(got), 0) == INV and L.sdm_get_world_occupied(h, None, 0, None, 0) == INV
    assert L.sdm_get_world_occupied(h, None, 0, C.byref(got), 2) == INV
    assert L.sdm_query_world_points(h, vp(xyz), -1, vp(out), 0) == INV and L.sdm_query_world_points(h, None, 2, vp(out), 0) == INV
    assert L.sdm_query_world_points(h, vp(xyz), 2, vp(out), 4) == INV and L.sdm_query_world_points(h, vp(xyz), 0, vp(out), 0) == 0
    for bad in ([0, 1, 1], [1, -1, 1], [1 << 14, 1 << 14, 2]):
        assert L.sdm_get_world_region(h, vp(lo), vp(np.array(bad, np.int32)), vp(words), 0) == INV, bad
    assert L.sdm_get_world_region(h, None, vp(sz), vp(words), 0) == INV and L.sdm_get_world_region(h, vp(lo), vp(sz), vp(words), 2) == INV
    assert got.value == -7
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    o["max_bricks"] = 0
    assert L.sdm_world_update(shard.h, vp(o)) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_get_world_info(shard.h, vp(info)) == INV and L.sdm_world_clear(shard.h) == INV
    shard.close()
