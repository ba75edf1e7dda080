"""sdm_world_changes_update / sdm_get_world_changes / sdm_get_world_change_cells / sdm_get_world_change_labels /
sdm_query_world_changes (include/sdm.h) against tests/world_changes_ref.py's BrickModel, bit for bit: info with its eleven
counters, the table with its floats, the five cell arrays, the three label arrays and the query at every listed cell and at
cells beside them.  The model is fed with what the map itself returns: voxels() and ring_state() for the block,
world_bricks() for the archive.

The block is a crafted state (shape_cases.crafted_state on a ring of the case's choice, one blind frame), the archive is
filled through world_import from the arrays of tests/world_changes_cases.py - that gives control of occ == 2, movable
tracks, absent bricks and stamps on the archive side; the block side reading occ == 2 is covered without a GPU
(tests/test_world_changes_ref.py).  Shape A (4 cells an axis) inside one brick or astride two on every axis, shape C
(8 x 4 x 128) with seams on all three axes through the block, shape B for the random pair."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import test_world_gpu as twg
from tests import world_changes_cases as cc
from tests import world_changes_ref as wcr
from tests.test_ground_gpu import _cells

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV, CAPACITY = 1, 4
NONE, UNLISTED = binding.WORLD_CHANGE_NONE, binding.WORLD_CHANGE_UNLISTED
CAN = 0x5A
CASES = cc.crafted()
RANDOM = cc.random_pair()


def block_of(c):
    """a map whose result array reads the case's block on the case's ring (test_world_gpu.crafted with the block given)"""
    cfg = sc.config(c["shape"])
    ring = sc.crafted_ring(cfg, c["steps"])
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    occ = c["occ"]
    g.load_state(sc.crafted_state(cfg, ring, _cells(occ == 1), _cells(occ == -1), tracks=c["track"][occ == 1], labels=c["label"][occ == 1]))
    g.set_ring_state(ring)
    twg.blind_frame(g, cfg, ring["last_pos"])
    assert g.ring_state()["moved_steps"] == [int(s) for s in c["steps"]]
    return g, cfg


def pair_of(c):
    g, cfg = block_of(c)
    g.world_import(c["hdr"], c["cells"])
    return g, cfg, binding.WorldChanges(g)


def got_of(w):
    table, info = w.regions()
    return w.cells() + (table,) + w.labels() + (info,)


def probes(ref):
    """world cells: every listed cell, the cells beside them on every axis, cells of no brick and beyond the int16 range"""
    own = ref.cells.astype(np.int64).reshape(-1, 3)
    beside = np.concatenate([own + d for d in np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1]])]) if len(own) else own
    far = np.array([[8 * 32768, 0, 0], [0, -8 * 32769, 0], [2 ** 31 - 1, 0, 0], [0, 0, -2 ** 31], [5, 5, 5]], np.int64)
    return np.concatenate([own, beside, far])


def check_query(g, w, ref, device=False):
    cells = probes(ref)
    want = ref.query(cells=cells)
    got = w.query(cells=cells)
    assert got.tobytes() == want.tobytes()
    n = len(ref.cells)
    assert np.array_equal(got["index"][:n], np.arange(n)) and np.array_equal(got["region"][:n], ref.region) and np.array_equal(got["cls"][:n], ref.cls)
    if not device:
        return
    src = cells.astype(np.int32)
    d_in = g.device_put(src)
    d_out = g.device_put(np.full(len(src) * 24 + 16, CAN, np.uint8))
    w.query(cells=d_in, on_device=True, n=len(src), out=d_out + 8)
    g.synchronize()
    out = g.device_download(d_out, len(src) * 24 + 16)
    assert (out[:8] == CAN).all() and (out[-8:] == CAN).all() and out[8:-8].tobytes() == want.tobytes()


def check_build(g, cfg, w, device=False, **kw):
    """one build on the map and in the restatement, fed with what the map itself returns"""
    ring, snap = twg.snapshot(g, cfg)
    hdr, cells = g.world_bricks()
    w.update(**kw)
    ref = wcr.BrickModel(snap, ring["moved_steps"], ring["global_time_stamp"], hdr, cells, int(g.world_info()["stamp"]),
                         np.float32(cfg["voxel_size"]), cfg["max_movable_track"], **kw)
    diff = wcr.difference(got_of(w), wcr.answer(ref))
    assert diff is None, (kw, diff)
    check_query(g, w, ref, device)
    return ref


def check_expect(ref, want):
    for name, v in want.items():
        if name.endswith("_min"):
            assert int(ref.info[name[:-4]]) >= v, (name, ref.info)
        else:
            assert int(ref.info[name]) == v, (name, int(ref.info[name]), v)


# ---- the crafted pairs, every build of each
@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_pairs(name):
    c = CASES[name]
    g, cfg, w = pair_of(c)
    for k, (kw, want) in enumerate(c["builds"]):
        ref = check_build(g, cfg, w, device=k == 0, **kw)
        check_expect(ref, want)                        # (the library's answer is the model's, bit for bit)
        if name.startswith("class table") and not any(kw.values()):
            for counter in binding.WORLD_CHANGES_COUNTERS:
                assert ref.info[counter] > 0, counter
    g.close()


# ---- random: every flag set, OLDER, masks, min_cells
def test_the_random_pair_under_every_flag_set():
    g, cfg, w = pair_of(RANDOM)
    seen = set()
    for kw, _ in RANDOM["builds"]:
        ref = check_build(g, cfg, w, **kw)
        seen.add(int(ref.info["flags"]))
        assert ref.info["n_cells"] > 200 and ref.info["n_regions_total"] > 20
    assert len(seen) == 18
    g.close()


# ---- the ranges of the getters, canaries behind every caller buffer
def test_getter_ranges_and_canaries():
    g, cfg, w = pair_of(RANDOM)
    ref = check_build(g, cfg, w, face_connected=True, min_cells=2)
    n, nr = len(ref.cells), len(ref.table)
    assert n > 100 and nr > 5 and (ref.region == UNLISTED).any()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = C.c_int64(-1)
    cols = (ref.cells, ref.now, ref.before, ref.cls, ref.region)
    for first, cap in ((0, n), (7, 20), (n - 3, 10), (n, 4), (n + 5, 4), (3, 0)):
        take = max(min(n - first, cap), 0)
        bufs = [np.full((cap + 2, 3), 0x5A5A5A5A, np.int32), np.full(cap + 2, 0xA5A5A5A5, np.uint32), np.full(cap + 2, 0x5A5A5A5A, np.uint32),
                np.full(cap + 2, CAN, np.uint8), np.full(cap + 2, 0xA5A5A5A5, np.uint32)]
        fill = [b.reshape(-1)[0] for b in bufs]
        assert L.sdm_get_world_change_cells(h, *[vp(b) for b in bufs], first, cap, C.byref(got)) == 0 and got.value == n
        for b, col, f in zip(bufs, cols, fill):
            assert np.array_equal(b[:take], col[first:first + take]) and (b[take:] == f).all()
    part = w.cells(first=5, cap=9)
    assert all(np.array_equal(a, col[5:14]) for a, col in zip(part, cols))
    # each array alone, and none
    for k, col in enumerate(cols):
        one = np.zeros(col.shape, col.dtype)
        args = [None] * 5
        args[k] = vp(one)
        assert L.sdm_get_world_change_cells(h, *args, 0, n, C.byref(got)) == 0 and np.array_equal(one, col)
    assert L.sdm_get_world_change_cells(h, None, None, None, None, None, 0, n, C.byref(got)) == 0 and got.value == n
    # the table: a cap below the count
    k32 = C.c_int32(-1)
    out = np.zeros(nr + 1, binding.WORLD_CHANGE_REGION)
    out.view(np.uint8)[:] = 0xA5
    assert L.sdm_get_world_changes(h, vp(out), nr - 2, C.byref(k32), None) == 0 and k32.value == nr
    assert out[:nr - 2].tobytes() == ref.table[:nr - 2].tobytes() and (out[nr - 2:].view(np.uint8) == 0xA5).all()
    assert L.sdm_get_world_changes(h, None, 0, C.byref(k32), None) == 0 and k32.value == nr
    # the label counters: each array alone, 8 bytes of canary behind it
    for k, want in enumerate((ref.appeared, ref.vanished, ref.relabelled)):
        one = np.full(257, 0xA5A5A5A5A5A5A5A5, np.uint64)
        args = [None] * 3
        args[k] = vp(one)
        assert L.sdm_get_world_change_labels(h, *args) == 0 and np.array_equal(one[:256], want) and one[256] == 0xA5A5A5A5A5A5A5A5
    assert ref.appeared.sum() > 0 and ref.vanished.sum() > 0 and ref.relabelled.sum() > 0
    # info alone
    info = np.zeros(2, binding.WORLD_CHANGES_INFO)
    info.view(np.uint8)[:] = 0xA5
    assert L.sdm_get_world_changes(h, None, 0, C.byref(k32), vp(info)) == 0
    assert info[0].tobytes() == ref.info.tobytes() and (info[1:].view(np.uint8) == 0xA5).all()
    g.close()


# ---- max_cells
def test_max_cells_one_below_the_count():
    g, cfg, w = pair_of(RANDOM)
    ref = check_build(g, cfg, w, by_label=True)
    n = int(ref.info["n_cells"])
    before = [a.tobytes() for a in got_of(w)]
    w.update(by_label=True, max_cells=n)          # exactly enough
    assert [a.tobytes() for a in got_of(w)] == before
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o = np.zeros(1, binding.WORLD_CHANGES_OPTIONS)
    o["flags"], o["min_cells"], o["max_cells"], o["labels"], o["classes"] = binding.WORLD_CHANGES_BY_LABEL, 1, n - 1, 0xFFFFFFFF, 0xE
    cap_err = L.sdm_world_changes_update(h, vp(o))
    assert cap_err == CAPACITY and b"max_cells" in L.sdm_last_error()
    info, k32, k64 = np.zeros(1, binding.WORLD_CHANGES_INFO), C.c_int32(-7), C.c_int64(-7)
    out = np.zeros(4, binding.WORLD_CHANGE_REGION)
    out.view(np.uint8)[:] = 0xA5
    xyz, wd = np.full((n + 2, 3), 0x5A5A5A5A, np.int32), np.full(n + 2, 0x5A5A5A5A, np.uint32)
    assert L.sdm_get_world_changes(h, vp(out), 4, C.byref(k32), vp(info)) == cap_err and k32.value == -7
    for name in binding.WORLD_CHANGES_COUNTERS + ("n_candidates", "n_bricks", "n_cells"):   # the true counts are still served
        assert info[name][0] == ref.info[name], name
    assert info["n_regions"][0] == 0 and info["n_regions_total"][0] == 0
    assert L.sdm_get_world_change_cells(h, vp(xyz), vp(wd), None, None, None, 0, n, C.byref(k64)) == cap_err and k64.value == n
    assert (out.view(np.uint8) == 0xA5).all() and (xyz == 0x5A5A5A5A).all() and (wd == 0x5A5A5A5A).all()
    res = np.zeros(1, binding.WORLD_CHANGE_RESULT)
    assert L.sdm_query_world_changes(h, None, vp(np.zeros(3, np.int32)), 1, vp(res), 0) == cap_err
    assert L.sdm_get_world_change_labels(h, vp(np.zeros(256, np.uint64)), None, None) == cap_err
    with pytest.raises(binding.SdmError):
        w.regions()
    w.update(by_label=True, max_cells=n + 1)      # the next build, with room
    assert [a.tobytes() for a in got_of(w)] == before
    g.close()


# ---- the query by point
def test_the_query_by_point_host_and_device():
    c = CASES["vanished shapes"]
    g, cfg, w = pair_of(c)
    ref = check_build(g, cfg, w, min_cells=3)
    size = np.float32(cfg["voxel_size"])
    cells = probes(ref)
    inside = (np.abs(cells) < 2 ** 17).all(axis=1)
    pts = np.concatenate([(cells[inside].astype(np.float32) + np.float32(0.5)) * size,
                          np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e7, 0, 0], [0, -3e7, 0]], np.float32)])
    want = ref.query(xyz=pts, voxel_size=size)
    got = w.query(xyz=pts)
    assert got.tobytes() == want.tobytes()
    assert (want["region"] == UNLISTED).any() and (want["region"] == NONE).any() and (want["region"] < len(ref.table)).any()
    assert (got["region"][-5:] == NONE).all() and (got["cls"][-5:] == NONE).all()
    d_in = g.device_put(pts)
    d_out = g.device_put(np.full(len(pts) * 24 + 16, CAN, np.uint8))
    w.query(xyz=d_in, on_device=True, n=len(pts), out=d_out + 8)
    g.synchronize()
    out = g.device_download(d_out, len(pts) * 24 + 16)
    assert (out[:8] == CAN).all() and (out[-8:] == CAN).all() and out[8:-8].tobytes() == want.tobytes()
    # n == 0
    assert len(w.query(cells=np.zeros((0, 3), np.int32))) == 0
    d_none = g.device_put(np.full(40, CAN, np.uint8))
    w.query(xyz=d_in, on_device=True, n=0, out=d_none + 8)
    g.synchronize()
    assert (g.device_download(d_none, 40) == CAN).all()
    g.close()


# ---- the build is a snapshot; after the archiving a second build of the same frame lists nothing
def test_the_build_is_a_snapshot_and_the_archiving_settles_the_difference():
    c = CASES["appeared shapes"]
    g, cfg, w = pair_of(c)
    ref = check_build(g, cfg, w, min_cells=2)
    cells = probes(ref)
    state = lambda: [a.tobytes() for a in got_of(w)] + [w.query(cells=cells).tobytes()]  # noqa: E731
    before = state()
    assert ref.info["n_cells"] > 50 and before[-1] == ref.query(cells=cells).tobytes()
    g.world_update()                                              # the difference is overwritten as the archive takes the block
    assert state() == before
    again = check_build(g, cfg, w, min_cells=2)                   # the same frame against what it has just written
    assert again.info["n_cells"] == 0 and again.info["n_bricks"] == 0 and len(again.table) == 0
    assert again.info["n_new_occupied"] == 0 and again.info["n_new_free"] == 0
    assert again.info["n_known_now"] == again.info["n_same_occupied"] + again.info["n_same_free"] == ref.info["n_known_now"]
    g.world_import(c["hdr"], c["cells"])                          # the old memory again: the same differences, a build with cells
    ref = check_build(g, cfg, w, min_cells=2, by_label=True)
    before = state()
    assert ref.info["n_cells"] > 50
    assert g.world_retain(bmin=(0, -1, 0), bmax=(3, 5, 8)) >= 0   # removes bricks and compacts the pool
    assert state() == before
    twg.blind_frame(g, cfg, g.ring_state()["last_pos"])           # a later frame
    assert state() == before
    g.world_clear()
    assert state() == before
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        w.update()
    assert state() == before                                      # (a refused build leaves the last one standing)
    g.close()


# ---- two runs, no side effects
def test_two_runs_give_the_same_bytes_and_map_and_archive_are_left_alone():
    g, cfg, w = pair_of(RANDOM)
    state = lambda: [a.tobytes() for a in g.world_bricks()] + [g.world_info().tobytes(), g.voxels().tobytes(), repr(g.ring_state())]  # noqa: E731
    before = state()
    runs = []
    for _ in range(2):
        ref = check_build(g, cfg, w, by_label=True, min_cells=2)
        runs.append([a.tobytes() for a in got_of(w)])
    assert runs[0] == runs[1] and ref.info["n_cells"] > 0 and ref.info["frame_stamp"] == g.ring_state()["global_time_stamp"]
    assert state() == before
    g.close()


# ---- an archive that holds no brick the block overlaps: everything known counts as new
def test_an_archive_elsewhere_makes_everything_new():
    c = CASES["class table"]
    g, cfg = block_of(c)
    far = cc.Pair("A", cc.steps_at(cfg, (40, 40, 40), (0, 0, 0)), archive=cc.word(cc.B)).case([])
    g.world_import(far["hdr"], far["cells"])
    ref = check_build(g, cfg, binding.WorldChanges(g))
    assert ref.info["n_cells"] == 0 and ref.info["n_known_before"] == 0 and ref.info["n_remembered"] == 0
    assert ref.info["n_known_now"] == ref.info["n_new_occupied"] + ref.info["n_new_free"] > 0
    g.close()


# ---- the argument checks
def test_argument_errors():
    c = CASES["class table"]
    g, cfg = block_of(c)
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o, info = np.zeros(1, binding.WORLD_CHANGES_OPTIONS), np.zeros(1, binding.WORLD_CHANGES_INFO)
    o["labels"], o["classes"] = 0xFFFFFFFF, 0xE
    out, res, cell = np.zeros(2, binding.WORLD_CHANGE_REGION), np.zeros(2, binding.WORLD_CHANGE_RESULT), np.zeros((2, 3), np.int32)
    k32, k64 = C.c_int32(-7), C.c_int64(-7)
    # before the archive has had an update or import; the getters and the query before any build
    assert L.sdm_world_changes_update(h, vp(o)) == INV and b"sdm_world_update first" in L.sdm_last_error()
    g.world_import(c["hdr"], c["cells"])
    assert L.sdm_get_world_changes(h, vp(out), 2, C.byref(k32), vp(info)) == INV and b"sdm_world_changes_update first" in L.sdm_last_error()
    assert L.sdm_get_world_change_cells(h, None, None, None, None, None, 0, 0, C.byref(k64)) == INV and b"sdm_world_changes_update first" in L.sdm_last_error()
    assert L.sdm_get_world_change_labels(h, None, None, None) == INV and L.sdm_query_world_changes(h, None, vp(cell), 2, vp(res), 0) == INV
    assert k32.value == -7 and k64.value == -7
    # the build's arguments
    assert L.sdm_world_changes_update(h, None) == INV and L.sdm_world_changes_update(None, vp(o)) == INV
    o["flags"] = 0x20
    assert L.sdm_world_changes_update(h, vp(o)) == INV and b"flag" in L.sdm_last_error()
    o["flags"], o["classes"] = 0, 0x1
    assert L.sdm_world_changes_update(h, vp(o)) == INV and b"class" in L.sdm_last_error()
    o["classes"] = 0x10
    assert L.sdm_world_changes_update(h, vp(o)) == INV and b"class" in L.sdm_last_error()
    o["classes"], o["pad"] = 0xE, (0, 1)
    assert L.sdm_world_changes_update(h, vp(o)) == INV and b"pad" in L.sdm_last_error()
    o["pad"], o["max_cells"] = 0, -1
    assert L.sdm_world_changes_update(h, vp(o)) == INV and b"max_cells" in L.sdm_last_error()
    o["max_cells"], o["max_last_stamp"] = 0, 0                    # without the flag the stamp is not read
    assert L.sdm_world_changes_update(h, vp(o)) == 0
    # the getters
    assert L.sdm_get_world_changes(h, vp(out), 2, C.byref(k32), vp(info)) == 0 and k32.value > 0 and info["n_cells"][0] > 0
    n = int(info["n_cells"][0])
    assert L.sdm_get_world_changes(h, vp(out), -1, C.byref(k32), None) == INV and L.sdm_get_world_changes(h, vp(out), 2, None, None) == INV
    assert L.sdm_get_world_changes(h, None, 1, C.byref(k32), None) == INV and L.sdm_get_world_changes(h, None, 0, C.byref(k32), None) == 0
    assert L.sdm_get_world_change_cells(h, None, None, None, None, None, -1, 0, C.byref(k64)) == INV
    assert L.sdm_get_world_change_cells(h, None, None, None, None, None, 0, -1, C.byref(k64)) == INV
    assert L.sdm_get_world_change_cells(h, None, None, None, None, None, 0, 0, None) == INV
    assert L.sdm_get_world_change_cells(h, None, None, None, None, None, 0, 0, C.byref(k64)) == 0 and k64.value == n
    assert L.sdm_get_world_change_labels(h, None, None, None) == 0
    # the query
    xyz = np.zeros((2, 3), np.float32)
    assert L.sdm_query_world_changes(h, vp(xyz), vp(cell), 2, vp(res), 0) == INV and L.sdm_query_world_changes(h, None, None, 2, vp(res), 0) == INV
    assert L.sdm_query_world_changes(h, None, None, 0, vp(res), 0) == INV and L.sdm_query_world_changes(h, None, vp(cell), -1, vp(res), 0) == INV
    assert L.sdm_query_world_changes(h, None, vp(cell), 2, None, 0) == INV and L.sdm_query_world_changes(h, None, vp(cell), 2, vp(res), 0x80) == INV
    assert L.sdm_query_world_changes(None, None, vp(cell), 2, vp(res), 0) == INV
    assert L.sdm_query_world_changes(h, None, vp(cell), 2, vp(res), 0) == 0 and res["region"].tolist() == [NONE, NONE]
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    o[:] = 0
    assert L.sdm_world_changes_update(shard.h, vp(o)) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_get_world_changes(shard.h, vp(out), 2, C.byref(k32), None) == INV
    assert L.sdm_get_world_change_cells(shard.h, None, None, None, None, None, 0, 0, C.byref(k64)) == INV
    assert L.sdm_get_world_change_labels(shard.h, None, None, None) == INV
    assert L.sdm_query_world_changes(shard.h, None, vp(cell), 2, vp(res), 0) == INV
    shard.close()
