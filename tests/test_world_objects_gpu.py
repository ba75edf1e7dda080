"""sdm_world_objects_update / sdm_get_world_objects / sdm_get_world_object_cells / sdm_get_world_object_labels /
sdm_query_world_objects (include/sdm.h) against tests/world_objects_ref.py's BrickModel, bit for bit: the cell list with
its words, the object index per cell, the table with its floats, the per-label counters and info.  The model is fed with
what world_bricks() of the same map returns.

The archive needs a map only as a handle: every case but the last feeds the hand-written bricks of
tests/world_objects_cases.py to world_import on a fresh map of shape A (4 cells an axis).  The crafted cases with their
closed forms, the random archive under 16 option sets and a box; the ranges of the getters; max_cells; the query; the
snapshot under retain, import and clear; reproducibility and no side effects; the argument checks; frames, world_update and
the objects of what they archived."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import test_world_gpu as twg
from tests import world_objects_cases as oc
from tests import world_objects_ref as wor

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV, CAPACITY = 1, 4
CFG = oc.CFG
SIZE = np.float32(CFG["voxel_size"])
NONE, UNLISTED = binding.WORLD_OBJECT_NONE, binding.WORLD_OBJECT_UNLISTED
CAN = 0x5A


def handle():
    return binding.SdmMap(CFG, PARAMS, synth.noise_table())


def world_of(c):
    g = handle()
    g.world_import(c["hdr"], c["cells"])
    return g


def got_of(g):
    cells, obj, words = g.world_object_cells()
    table, info = g.world_objects()
    lab_cells, lab_objs = g.world_object_labels()
    return cells, obj, words, table, lab_cells, lab_objs, info


def check_build(g, size=SIZE, mm=oc.MM, **kw):
    """one build on the map and in the restatement, fed with what the map itself returns"""
    hdr, cells = g.world_bricks()
    g.world_objects_update(**kw)
    ref = wor.BrickModel(hdr, cells, size, mm, stamp=int(g.world_info()["stamp"]), **kw)
    diff = wor.difference(got_of(g), wor.answer(ref))
    assert diff is None, (kw, diff)
    return ref


CASES = oc.crafted()
RANDOM = oc.random_archive()


# ---- the crafted cases, every build of each
@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_archives(name):
    c = CASES[name]
    g = world_of(c)
    for k, (kw, _) in enumerate(c["builds"]):
        ref = check_build(g, **kw)
        oc.check_closed_forms(name, c, k, ref)     # (the library's answer is the model's, bit for bit)
    g.close()


# ---- random: 16 option sets and a box
def test_the_random_archive_under_every_option():
    g = world_of(dict(hdr=RANDOM[0], cells=RANDOM[1]))
    seen = set()
    for kw in oc.random_variants():
        ref = check_build(g, **kw)
        seen.add((int(ref.info["flags"]), int(ref.info["min_cells"])))
        assert ref.info["n_cells"] > 1000
    assert len(seen) == 17
    g.close()


# ---- the ranges of the getters
def test_getter_ranges_and_canaries():
    g = world_of(dict(hdr=RANDOM[0], cells=RANDOM[1]))
    ref = check_build(g, face_connected=True, min_cells=2)
    n, nc = len(ref.cells), len(ref.table)
    assert n > 100 and nc > 5
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = C.c_int64(-1)
    for first, cap in ((0, n), (7, 20), (n - 3, 10), (n, 4), (n + 5, 4), (3, 0)):
        take = max(min(n - first, cap), 0)
        xyz, ob, wd = np.full((cap + 2, 3), 0x5A5A5A5A, np.int32), np.full(cap + 2, 0xA5A5A5A5, np.uint32), np.full(cap + 2, 0x5A5A5A5A, np.uint32)
        assert L.sdm_get_world_object_cells(h, vp(xyz), vp(ob), vp(wd), first, cap, C.byref(got)) == 0 and got.value == n
        assert np.array_equal(xyz[:take], ref.cells[first:first + take]) and (xyz[take:] == 0x5A5A5A5A).all()
        assert np.array_equal(ob[:take], ref.object[first:first + take]) and (ob[take:] == 0xA5A5A5A5).all()
        assert np.array_equal(wd[:take], ref.words[first:first + take]) and (wd[take:] == 0x5A5A5A5A).all()
    part = g.world_object_cells(first=5, cap=9)
    assert np.array_equal(part[0], ref.cells[5:14]) and np.array_equal(part[1], ref.object[5:14]) and np.array_equal(part[2], ref.words[5:14])
    # each array alone
    wd = np.zeros(n, np.uint32)
    assert L.sdm_get_world_object_cells(h, None, None, vp(wd), 0, n, C.byref(got)) == 0 and np.array_equal(wd, ref.words)
    xyz = np.zeros((n, 3), np.int32)
    assert L.sdm_get_world_object_cells(h, vp(xyz), None, None, 0, n, C.byref(got)) == 0 and np.array_equal(xyz, ref.cells)
    assert L.sdm_get_world_object_cells(h, None, None, None, 0, n, C.byref(got)) == 0 and got.value == n
    # the table: a cap below the count
    k32 = C.c_int32(-1)
    out = np.zeros(nc + 1, binding.WORLD_OBJECT)
    out.view(np.uint8)[:] = 0xA5
    assert L.sdm_get_world_objects(h, vp(out), nc - 2, C.byref(k32), None) == 0 and k32.value == nc
    assert out[:nc - 2].tobytes() == ref.table[:nc - 2].tobytes() and (out[nc - 2:].view(np.uint8) == 0xA5).all()
    assert L.sdm_get_world_objects(h, None, 0, C.byref(k32), None) == 0 and k32.value == nc
    # the label counters: either array alone
    lc, lo = np.zeros(256, np.uint64), np.zeros(256, np.uint32)
    assert L.sdm_get_world_object_labels(h, vp(lc), None) == 0 and L.sdm_get_world_object_labels(h, None, vp(lo)) == 0
    assert np.array_equal(lc, ref.label_cells) and np.array_equal(lo, ref.label_objects)
    # one object's members
    i = int(np.argmax(ref.table["n_cells"]))
    cells, words = g.world_object_members(i)
    assert np.array_equal(cells, ref.cells[ref.object == i]) and np.array_equal(words, ref.words[ref.object == i]) and len(cells) == ref.table["n_cells"][i]
    g.close()


# ---- max_cells
def test_max_cells_one_below_the_count():
    g = world_of(dict(hdr=RANDOM[0], cells=RANDOM[1]))
    ref = check_build(g, by_track=True)
    n = int(ref.info["n_cells"])
    before = [a.tobytes() for a in got_of(g)]
    g.world_objects_update(by_track=True, max_cells=n)          # exactly enough
    assert [a.tobytes() for a in got_of(g)] == before
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o = np.zeros(1, binding.WORLD_OBJECTS_OPTIONS)
    o["flags"], o["min_cells"], o["max_cells"], o["labels"] = binding.WORLD_OBJECTS_BY_TRACK, 1, n - 1, 0xFFFFFFFF
    cap_err = L.sdm_world_objects_update(h, vp(o))
    assert cap_err == CAPACITY and b"max_cells" in L.sdm_last_error()
    info, k32, k64 = np.zeros(1, binding.WORLD_OBJECTS_INFO), C.c_int32(-7), C.c_int64(-7)
    out = np.zeros(4, binding.WORLD_OBJECT)
    out.view(np.uint8)[:] = 0xA5
    xyz, ob, wd = np.full((n + 2, 3), 0x5A5A5A5A, np.int32), np.full(n + 2, 0xA5A5A5A5, np.uint32), np.full(n + 2, 0x5A5A5A5A, np.uint32)
    assert L.sdm_get_world_objects(h, vp(out), 4, C.byref(k32), vp(info)) == cap_err and k32.value == -7
    assert info["n_cells"][0] == n and info["n_bricks"][0] == len(RANDOM[0]) and info["n_objects"][0] == 0 and info["n_objects_total"][0] == 0
    assert info["n_guessed"][0] == ref.info["n_guessed"] > 0
    assert L.sdm_get_world_object_cells(h, vp(xyz), vp(ob), vp(wd), 0, n, C.byref(k64)) == cap_err and k64.value == n
    assert (out.view(np.uint8) == 0xA5).all() and (xyz == 0x5A5A5A5A).all() and (ob == 0xA5A5A5A5).all() and (wd == 0x5A5A5A5A).all()
    res = np.zeros(1, binding.WORLD_OBJECT_RESULT)
    assert L.sdm_query_world_objects(h, None, vp(np.zeros(3, np.int32)), 1, vp(res), 0) == cap_err
    assert L.sdm_get_world_object_labels(h, vp(np.zeros(256, np.uint64)), None) == cap_err
    with pytest.raises(binding.SdmError):
        g.world_objects()
    g.world_objects_update(by_track=True, max_cells=n + 1)      # the next build, with room
    assert [a.tobytes() for a in got_of(g)] == before
    g.close()


# ---- the query
def probes(ref, seed=5):
    """world cells: counted cells (listed and not), cells of field bricks that do not count, cells of no brick, cells of
    bricks beyond the int16 range"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(ref.cells), min(200, len(ref.cells)), replace=False)
    base = ref.coords.astype(np.int64) * 8
    anywhere = base[rng.integers(0, len(base), 200)] + rng.integers(0, 8, (200, 3))
    far = np.array([[base[:, 0].max() + 16, base[0, 1], base[0, 2]], [0, 0, base[:, 2].min() - 9], [8 * 32768, 0, 0], [0, -8 * 32769, 0],
                    [2 ** 31 - 1, 0, 0], [0, 0, -2 ** 31]], np.int64)
    return np.concatenate([ref.cells[pick].astype(np.int64), anywhere, far])


def test_the_query_points_and_cells_host_and_device():
    g = world_of(dict(hdr=RANDOM[0], cells=RANDOM[1]))
    ref = check_build(g, min_cells=3)
    cells = probes(ref)
    want = ref.query(cells=cells)
    got = g.query_world_objects(cells=cells)
    assert got.tobytes() == want.tobytes()
    assert (want["object"] == UNLISTED).any() and (want["object"] == NONE).any() and (want["object"] < len(ref.table)).any()
    assert (got["index"][:200] != NONE).all() and np.array_equal(ref.object[got["index"][:200]], got["object"][:200])
    # points: the middle of each cell within reach, and what is no point of the world
    inside = (np.abs(cells) < 2 ** 17).all(axis=1)
    pts = np.concatenate([(cells[inside].astype(np.float32) + np.float32(0.5)) * SIZE,
                          np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e7, 0, 0], [0, -3e7, 0]], np.float32)])
    want_p = ref.query(xyz=pts, voxel_size=SIZE)
    got_p = g.query_world_objects(xyz=pts)
    assert got_p.tobytes() == want_p.tobytes()
    assert np.array_equal(got_p["index"][:int(inside.sum())], want["index"][inside]) and (got_p["object"][-5:] == NONE).all()
    # device mode, 8 bytes of canary before and behind
    for kw, src, expect in (("cells", cells.astype(np.int32), want), ("xyz", pts, want_p)):
        n = len(src)
        d_in = g.device_put(src)
        d_out = g.device_put(np.full(n * 24 + 16, CAN, np.uint8))
        g.query_world_objects(**{kw: d_in}, on_device=True, n=n, out=d_out + 8)
        g.synchronize()
        out = g.device_download(d_out, n * 24 + 16)
        assert (out[:8] == CAN).all() and (out[-8:] == CAN).all() and out[8:-8].tobytes() == expect.tobytes()
    # n == 0
    assert len(g.query_world_objects(cells=np.zeros((0, 3), np.int32))) == 0
    d_none = g.device_put(np.full(40, CAN, np.uint8))
    g.query_world_objects(cells=d_in, on_device=True, n=0, out=d_none + 8)
    g.synchronize()
    assert (g.device_download(d_none, 40) == CAN).all()
    g.close()


# ---- the build is a snapshot
def test_the_build_is_a_snapshot():
    g = world_of(dict(hdr=RANDOM[0], cells=RANDOM[1]))
    ref = check_build(g, min_cells=2)
    cells = probes(ref)
    state = lambda: [a.tobytes() for a in got_of(g)] + [g.query_world_objects(cells=cells).tobytes()]  # noqa: E731
    before = state()
    assert before[-1] == ref.query(cells=cells).tobytes()
    assert g.world_retain(bmin=(0, -1, 0), bmax=(5, 5, 5)) > 0          # removes bricks and compacts the pool
    assert state() == before
    other = CASES["serpentine tube"]
    g.world_import(other["hdr"], other["cells"], offset=(3, 0, -5))
    assert state() == before
    g.world_clear()
    assert state() == before
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        g.world_objects_update()
    assert state() == before                                            # (a refused build leaves the last one standing)
    g.world_import(other["hdr"], other["cells"])                        # a new build sees the new archive
    check_build(g, **other["builds"][0][0])
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
        ref = check_build(g, size=np.float32(cfg["voxel_size"]), mm=cfg["max_movable_track"], by_track=True)
        runs.append([a.tobytes() for a in got_of(g)])
    assert runs[0] == runs[1] and ref.info["n_cells"] > 0 and ref.info["stamp"] == g.ring_state()["global_time_stamp"]
    assert state() == before
    g.close()


# ---- integration: frames, world_update, the objects of what they archived, each found again by its first cell
def test_frames_archive_objects_that_the_query_finds_again():
    cfg = sc.config("B")
    steps = np.array(sc.crafted_steps(cfg), np.int64)
    g = twg.crafted(cfg, steps, seed=12)
    g.world_update()
    for _ in range(2):                                   # the camera drives off along z; the archive keeps what it leaves
        steps[2] += int(twg.dims(cfg)[2]) // 8
        twg.blind_frame(g, cfg, twg.cam_of(cfg, steps))
        g.world_update()
    ref = check_build(g, size=np.float32(cfg["voxel_size"]), mm=cfg["max_movable_track"], min_cells=2)
    table, info = g.world_objects()
    assert len(table) > 1 and info["n_objects_total"] > len(table) and info["stamp"] == g.ring_state()["global_time_stamp"]
    res = g.query_world_objects(cells=table["first_cell"])
    assert np.array_equal(res["object"], np.arange(len(table))) and np.array_equal(res["index"], table["first_index"])
    g.close()


# ---- the argument checks
def test_argument_errors():
    g = handle()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o, info = np.zeros(1, binding.WORLD_OBJECTS_OPTIONS), np.zeros(1, binding.WORLD_OBJECTS_INFO)
    o["labels"] = 0xFFFFFFFF
    out, res, cell = np.zeros(2, binding.WORLD_OBJECT), np.zeros(2, binding.WORLD_OBJECT_RESULT), np.zeros((2, 3), np.int32)
    k32, k64 = C.c_int32(-7), C.c_int64(-7)
    # before the archive has had an update or import; the getters and the query before any build
    assert L.sdm_world_objects_update(h, vp(o)) == INV and b"sdm_world_update first" in L.sdm_last_error()
    c = CASES["full brick"]
    g.world_import(c["hdr"], c["cells"])
    assert L.sdm_get_world_objects(h, vp(out), 2, C.byref(k32), vp(info)) == INV and b"sdm_world_objects_update first" in L.sdm_last_error()
    assert L.sdm_get_world_object_cells(h, None, None, None, 0, 0, C.byref(k64)) == INV and b"sdm_world_objects_update first" in L.sdm_last_error()
    assert L.sdm_get_world_object_labels(h, None, None) == INV and L.sdm_query_world_objects(h, None, vp(cell), 2, vp(res), 0) == INV
    assert k32.value == -7 and k64.value == -7
    # the build's arguments
    assert L.sdm_world_objects_update(h, None) == INV and L.sdm_world_objects_update(None, vp(o)) == INV
    o["flags"] = 0x40
    assert L.sdm_world_objects_update(h, vp(o)) == INV and b"flag" in L.sdm_last_error()
    o["flags"] = binding.WORLD_OBJECTS_STATIC_ONLY | binding.WORLD_OBJECTS_MOVABLE_ONLY
    assert L.sdm_world_objects_update(h, vp(o)) == INV and b"MOVABLE_ONLY" in L.sdm_last_error()
    o["flags"], o["max_cells"] = 0, -1
    assert L.sdm_world_objects_update(h, vp(o)) == INV and b"max_cells" in L.sdm_last_error()
    o["max_cells"], o["bmin"], o["bmax"] = 0, (5, 5, 5), (4, 4, 4)       # without the flag the box is not read
    assert L.sdm_world_objects_update(h, vp(o)) == 0
    # the getters
    assert L.sdm_get_world_objects(h, vp(out), 2, C.byref(k32), vp(info)) == 0 and k32.value == 1 and info["n_cells"][0] == 512
    assert L.sdm_get_world_objects(h, vp(out), -1, C.byref(k32), None) == INV and L.sdm_get_world_objects(h, vp(out), 2, None, None) == INV
    assert L.sdm_get_world_objects(h, None, 1, C.byref(k32), None) == INV and L.sdm_get_world_objects(h, None, 0, C.byref(k32), None) == 0
    assert L.sdm_get_world_object_cells(h, None, None, None, -1, 0, C.byref(k64)) == INV and L.sdm_get_world_object_cells(h, None, None, None, 0, -1, C.byref(k64)) == INV
    assert L.sdm_get_world_object_cells(h, None, None, None, 0, 0, None) == INV
    assert L.sdm_get_world_object_cells(h, None, None, None, 0, 0, C.byref(k64)) == 0 and k64.value == 512
    assert L.sdm_get_world_object_labels(h, None, None) == 0
    # the query
    xyz = np.zeros((2, 3), np.float32)
    assert L.sdm_query_world_objects(h, vp(xyz), vp(cell), 2, vp(res), 0) == INV and L.sdm_query_world_objects(h, None, None, 2, vp(res), 0) == INV
    assert L.sdm_query_world_objects(h, None, None, 0, vp(res), 0) == INV and L.sdm_query_world_objects(h, None, vp(cell), -1, vp(res), 0) == INV
    assert L.sdm_query_world_objects(h, None, vp(cell), 2, None, 0) == INV and L.sdm_query_world_objects(h, None, vp(cell), 2, vp(res), 0x80) == INV
    assert L.sdm_query_world_objects(None, None, vp(cell), 2, vp(res), 0) == INV
    assert L.sdm_query_world_objects(h, None, vp(cell), 2, vp(res), 0) == 0 and res["object"].tolist() == [0, 0] and res["index"].tolist() == [0, 0]
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    o[:] = 0
    assert L.sdm_world_objects_update(shard.h, vp(o)) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_get_world_objects(shard.h, vp(out), 2, C.byref(k32), None) == INV
    assert L.sdm_get_world_object_cells(shard.h, None, None, None, 0, 0, C.byref(k64)) == INV
    assert L.sdm_get_world_object_labels(shard.h, None, None) == INV
    assert L.sdm_query_world_objects(shard.h, None, vp(cell), 2, vp(res), 0) == INV
    shard.close()
