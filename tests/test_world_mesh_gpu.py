"""sdm_world_mesh_update / sdm_get_world_mesh_info / sdm_get_world_mesh_faces / sdm_get_world_mesh_vertices /
sdm_world_mesh_device (include/sdm.h) against tests/world_mesh_ref.py's BrickModel, bit for bit: coords, faces, quads,
corners, xyz and info.  The model is fed with what world_bricks() of the same map returns.

The archive needs a map only as a handle: every case but the last two feeds the hand-written bricks of
tests/world_mesh_cases.py to world_import on a fresh map of shape A (4 cells an axis).  The crafted cases with their closed
forms, the random archive under every legal flag combination without and with a box, empty fields; the getters' ranges; the
caps; the snapshot under retain, import, clear and update; reproducibility and no side effects; the device pointers; the
argument checks; frames whose camera leaves what it archived; the PLY export."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import test_world_gpu as twg
from tests import world_mesh_cases as mc
from tests import world_mesh_ref as wmr
from tests.test_world_mesh_ref import check_closed, check_divergence, check_expect, check_normals, check_order

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV, CAPACITY = 1, 4
CFG = mc.CFG
SIZE = np.float32(CFG["voxel_size"])
MM = mc.MM
CRAFTED = mc.crafted()
vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def handle():
    return binding.SdmMap(CFG, PARAMS, synth.noise_table())


def world_of(c):
    g = handle()
    g.world_import(c["hdr"], c["cells"])
    return g


def model_of(g, max_movable=MM, voxel_size=SIZE, **kw):
    hdr, cells = g.world_bricks()
    return wmr.answer(wmr.BrickModel(hdr, cells, max_movable, stamp=int(g.world_info()["stamp"]), voxel_size=voxel_size, **kw))


def check_build(g, max_movable=MM, voxel_size=SIZE, **kw):
    """one build on the map and in the restatement, fed with what the map itself returns"""
    ref = model_of(g, max_movable, voxel_size, **kw)
    g.world_mesh_update(**kw)
    diff = wmr.difference(g.world_mesh(), ref)
    assert diff is None, diff
    return ref


def mesh_bytes(g):
    m = g.world_mesh()
    return [np.asarray(m[k]).tobytes() for k in ("coords", "faces", "quads", "corners", "xyz", "info")]


# ---- the crafted cases
@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_archives(name):
    c = CRAFTED[name]
    g = world_of(c)
    ref = check_build(g, **c["kw"])
    check_expect(c, ref), check_order(ref), check_normals(ref)     # (the library's answer is the model's, bit for bit)
    g.close()


# ---- random, every legal flag combination, without and with a box
def test_the_random_archive_under_every_option():
    hdr, cells = mc.random_archive()
    g = world_of(dict(hdr=hdr, cells=cells))
    seen = set()
    for kw in mc.random_variants():
        ref = check_build(g, **kw)
        if not kw["skip_unknown_faces"] and not kw["skip_absent_faces"] and kw["box"] is None:
            check_closed(ref), check_divergence(ref)
        seen.add(int(ref["info"]["options"]["flags"]))
    assert len(seen) == 48
    g.close()


# ---- empty fields
def test_an_empty_field_is_no_error():
    c = CRAFTED["x wrap"]
    for empty_archive in (False, True):
        g = world_of(c)
        if empty_archive:
            assert g.world_retain(bmin=(0, 0, 0), bmax=(-1, 0, 0)) == 1 and g.world_info()["n_bricks"] == 0
            boxes = [None]
        else:
            boxes = [((100, 100, 100), (101, 101, 101)), ((0, 0, 0), (0, -1, 0))]
        for box in boxes:
            check_build(g, box=box)
            m = g.world_mesh()
            assert m["coords"].shape == (0, 3) and len(m["faces"]) == 0 and len(m["corners"]) == 0
            assert all(m["info"][k] == 0 for k in ("n_bricks", "n_vertex_bricks", "n_faces", "n_vertices", "n_solid"))
        if not empty_archive:   # the next build, without the box, has the brick again
            assert check_build(g)["info"]["n_faces"] == 12
        g.close()


# ---- the getters' ranges
def test_getter_ranges_and_canaries():
    c = CRAFTED["pillars all"]
    g = world_of(c)
    ref = check_build(g)
    nf, nv, nb = len(ref["faces"]), len(ref["corners"]), len(ref["coords"])
    assert nf > 40 and nv > 40 and nb == 17
    L, h = g.L, g.h
    got = C.c_int64(-1)
    for first, cap in ((0, nf), (3, 5), (nf - 2, 6), (nf, 4), (nf + 5, 4), (2, 0)):
        take = max(min(nf - first, cap), 0)
        cb = np.full((nb + 2, 3), 0x5A5A, np.int16)
        fb, qb = np.full((cap + 2) * 12, 0xA5, np.uint8), np.full((cap + 2, 4), 0xA5A5A5A5, np.uint32)
        assert L.sdm_get_world_mesh_faces(h, vp(cb), vp(fb), vp(qb), first, cap, C.byref(got)) == 0 and got.value == nf
        assert fb[:take * 12].tobytes() == ref["faces"][first:first + take].tobytes() and (fb[take * 12:] == 0xA5).all()
        assert np.array_equal(qb[:take], ref["quads"][first:first + take]) and (qb[take:] == 0xA5A5A5A5).all()
        if first == 0:      # every row of the field, whatever cap is
            assert np.array_equal(cb[:nb], ref["coords"]) and (cb[nb:] == 0x5A5A).all()
        else:
            assert (cb == 0x5A5A).all()
    for first, cap in ((0, nv), (4, 7), (nv - 1, 3), (nv, 2), (1, 0)):
        take = max(min(nv - first, cap), 0)
        kb, xb = np.full((cap + 2, 3), 0x5A5A5A5A, np.int32), np.full((cap + 2, 3), 7.5, np.float32)
        assert L.sdm_get_world_mesh_vertices(h, vp(kb), vp(xb), first, cap, C.byref(got)) == 0 and got.value == nv
        assert np.array_equal(kb[:take], ref["corners"][first:first + take]) and (kb[take:] == 0x5A5A5A5A).all()
        assert xb[:take].tobytes() == ref["xyz"][first:first + take].tobytes() and (xb[take:] == 7.5).all()
    # each array alone, and none
    xb = np.zeros((nv, 3), np.float32)
    assert L.sdm_get_world_mesh_vertices(h, None, vp(xb), 0, nv, C.byref(got)) == 0 and xb.tobytes() == ref["xyz"].tobytes()
    qb = np.zeros((nf, 4), np.uint32)
    assert L.sdm_get_world_mesh_faces(h, None, None, vp(qb), 0, nf, C.byref(got)) == 0 and np.array_equal(qb, ref["quads"])
    assert L.sdm_get_world_mesh_faces(h, None, None, None, 0, 0, C.byref(got)) == 0 and got.value == nf
    # without a box row r is row r of world_bricks()
    hdr, _ = g.world_bricks()
    assert np.array_equal(ref["coords"], np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int16))
    g.close()


# ---- the caps
def test_caps_refuse_and_write_nothing():
    hdr, cells = mc.random_archive()
    g = world_of(dict(hdr=hdr, cells=cells))
    big = check_build(g, box=mc.RANDOM_BOX)                            # a build with room: lists the capped builds must not touch
    nf, nv = int(big["info"]["n_faces"]), int(big["info"]["n_vertices"])
    L, h = g.L, g.h
    got = C.c_int64(-1)
    for kw in (dict(max_faces=nf - 1), dict(max_vertices=nv - 1), dict(max_faces=1, max_vertices=1)):
        with pytest.raises(binding.SdmError, match="SDM_ERR_CAPACITY"):
            g.world_mesh_update(box=mc.RANDOM_BOX, **kw)
        want = model_of(g, box=mc.RANDOM_BOX, **kw)["info"]
        assert g.world_mesh_info().tobytes() == want.tobytes() and want["n_faces"] == nf   # the true counts
        fb, qb, kb = np.full(24, 0xA5, np.uint8), np.full((2, 4), 0xA5A5A5A5, np.uint32), np.full((2, 3), 0x5A5A5A5A, np.int32)
        assert L.sdm_get_world_mesh_faces(h, None, vp(fb), vp(qb), 0, 2, C.byref(got)) == CAPACITY and got.value == nf
        assert L.sdm_get_world_mesh_vertices(h, vp(kb), None, 0, 2, C.byref(got)) == CAPACITY and got.value == nv
        assert (fb == 0xA5).all() and (qb == 0xA5A5A5A5).all() and (kb == 0x5A5A5A5A).all()
        with pytest.raises(binding.SdmError, match="SDM_ERR_CAPACITY"):
            g.world_mesh_device()
    check_build(g, box=mc.RANDOM_BOX, max_faces=nf, max_vertices=nv)   # exactly enough
    whole = check_build(g)                                             # a larger build, then a smaller one
    assert whole["info"]["n_faces"] > nf
    check_build(g, box=((0, 0, 1), (0, 0, 1)), static_only=True)
    g.close()


# ---- the build is a snapshot
def test_the_build_is_a_snapshot():
    hdr, cells = mc.random_archive()
    g = world_of(dict(hdr=hdr, cells=cells))
    check_build(g, observed_only=True)
    before = mesh_bytes(g)
    assert g.world_retain(bmin=(0, -1, 0), bmax=(5, 5, 5)) > 0          # removes bricks and compacts the pool
    assert mesh_bytes(g) == before
    other = CRAFTED["cube 2 x 2 x 2"]
    g.world_import(other["hdr"], other["cells"], offset=(3, 0, -5))
    assert mesh_bytes(g) == before
    g.world_clear()
    assert mesh_bytes(g) == before
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        g.world_mesh_update()
    assert mesh_bytes(g) == before                                      # (a refused build leaves the last one standing)
    g.world_import(other["hdr"], other["cells"])                        # a new build sees the new archive
    ref = check_build(g)
    check_expect(other, ref)
    g.close()


def block_map(seed):
    """a map of shape B with a crafted state, one frame issued and archived -> (map, cfg)"""
    cfg = sc.config("B")
    g = twg.crafted(cfg, sc.crafted_steps(cfg), seed=seed)
    g.world_update()
    return g, cfg


# ---- two runs, no side effects; the snapshot under an update; the device pointers
def test_two_runs_give_the_same_bytes_and_the_map_is_left_alone():
    g, cfg = block_map(12)
    size = np.float32(cfg["voxel_size"])
    state = lambda: [a.tobytes() for a in g.world_bricks()] + [g.world_info().tobytes(), g.voxels().tobytes(), repr(g.ring_state())]  # noqa: E731
    before = state()
    runs = []
    for _ in range(2):
        ref = check_build(g, max_movable=cfg["max_movable_track"], voxel_size=size)
        runs.append(mesh_bytes(g))
    assert runs[0] == runs[1] and ref["info"]["n_faces"] > 0 and ref["info"]["stamp"] == g.ring_state()["global_time_stamp"]
    assert state() == before
    # the device pointers, read back
    nf, nv = len(ref["faces"]), len(ref["corners"])
    f, q, k = g.world_mesh_device()
    g.synchronize()
    assert g.device_download(f, nf * 12).tobytes() == ref["faces"].tobytes()
    assert g.device_download(q, nf * 16).tobytes() == ref["quads"].tobytes()
    assert g.device_download(k, nv * 12).tobytes() == ref["corners"].tobytes()
    g.world_update()                                                    # the archive moves on, the snapshot stays
    assert mesh_bytes(g) == runs[0]
    g.close()


# ---- integration: frames whose camera leaves what it archived
def test_frames_then_one_world_mesh():
    cfg = sc.config("B")
    N = twg.dims(cfg)
    steps = np.array(sc.crafted_steps(cfg), np.int64)
    g = twg.crafted(cfg, steps.tolist(), seed=5)
    g.world_update()
    first = int(g.world_info()["n_bricks"])
    for _ in range(2):                                   # the camera drives off along z; what comes in is unobserved
        steps[2] += int(N[2]) // 8
        twg.blind_frame(g, cfg, twg.cam_of(cfg, steps))
        g.world_update()
    assert int(g.world_info()["n_bricks"]) >= first
    ref = check_build(g, max_movable=cfg["max_movable_track"], voxel_size=np.float32(cfg["voxel_size"]))
    check_order(ref), check_normals(ref), check_closed(ref), check_divergence(ref)
    g0 = steps - (N >> 1)                                # world cell of the block's cell (0, 0, 0)
    assert ref["info"]["n_faces"] > 0 and (ref["corners"][:, 2] < g0[2]).any()     # faces of what the block has left
    g.close()


# ---- the PLY export
def test_save_world_ply(tmp_path):
    c = CRAFTED["checkerboard"]
    g = world_of(c)
    path = tmp_path / "world.ply"
    mesh = g.save_world_ply(str(path), skip_absent_faces=True)
    ref = model_of(g, skip_absent_faces=True)
    assert wmr.difference(mesh, ref) is None
    lines = path.read_text().split("\n")
    end = lines.index("end_header")
    assert "element vertex %d" % len(ref["corners"]) in lines[:end] and "element face %d" % (2 * len(ref["faces"])) in lines[:end]
    body = lines[end + 1:]
    nv, nt = len(ref["corners"]), 2 * len(ref["faces"])
    xyz = np.array([l.split() for l in body[:nv]], np.float32)
    tri = np.array([l.split() for l in body[nv:nv + nt]], np.int64)
    assert xyz.tobytes() == ref["xyz"].tobytes() and (tri[:, 0] == 3).all()
    assert np.array_equal(tri[:, 1:], binding.mesh_triangles(ref["quads"]))
    g.close()


# ---- the argument checks
def test_argument_errors():
    g = handle()
    L, h = g.L, g.h
    o, info = np.zeros(1, binding.WORLD_MESH_OPTIONS), np.zeros(1, binding.WORLD_MESH_INFO)
    o["track"] = -1
    o["labels"] = 0xFFFFFFFF
    k64 = C.c_int64(-7)
    p = [C.c_void_p() for _ in range(3)]
    # before the archive has had an update or import; the getters before any build
    assert L.sdm_world_mesh_update(h, vp(o)) == INV and b"sdm_world_update first" in L.sdm_last_error()
    c = CRAFTED["x wrap"]
    g.world_import(c["hdr"], c["cells"])
    assert L.sdm_get_world_mesh_info(h, vp(info)) == INV and b"sdm_world_mesh_update first" in L.sdm_last_error()
    assert L.sdm_get_world_mesh_faces(h, None, None, None, 0, 0, C.byref(k64)) == INV and b"sdm_world_mesh_update first" in L.sdm_last_error()
    assert L.sdm_get_world_mesh_vertices(h, None, None, 0, 0, C.byref(k64)) == INV and k64.value == -7
    assert L.sdm_world_mesh_device(h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])) == INV
    # the build's arguments
    assert L.sdm_world_mesh_update(None, vp(o)) == INV and L.sdm_world_mesh_update(h, None) == INV
    o["flags"] = 0x40
    assert L.sdm_world_mesh_update(h, vp(o)) == INV and b"flag" in L.sdm_last_error()
    o["flags"] = binding.WORLD_MESH_STATIC_ONLY | binding.WORLD_MESH_MOVABLE_ONLY
    assert L.sdm_world_mesh_update(h, vp(o)) == INV and b"both" in L.sdm_last_error()
    o["flags"] = 0
    for bad in (-2, 65536):
        o["track"] = bad
        assert L.sdm_world_mesh_update(h, vp(o)) == INV and b"track" in L.sdm_last_error()
    o["track"] = -1
    for field in ("max_faces", "max_vertices"):
        o[field] = -1
        assert L.sdm_world_mesh_update(h, vp(o)) == INV and b"cap" in L.sdm_last_error()
        o[field] = 0
    o["bmin"], o["bmax"] = (5, 5, 5), (4, 4, 4)                       # without the flag the box is not read
    assert L.sdm_world_mesh_update(h, vp(o)) == 0
    # the getters
    assert L.sdm_get_world_mesh_info(h, vp(info)) == 0 and info["n_faces"][0] == 12 and info["n_bricks"][0] == 1
    assert L.sdm_get_world_mesh_info(h, None) == INV and L.sdm_get_world_mesh_info(None, vp(info)) == INV
    for first, cap in ((-1, 0), (0, -1)):
        assert L.sdm_get_world_mesh_faces(h, None, None, None, first, cap, C.byref(k64)) == INV
        assert L.sdm_get_world_mesh_vertices(h, None, None, first, cap, C.byref(k64)) == INV
    assert L.sdm_get_world_mesh_faces(h, None, None, None, 0, 0, None) == INV and L.sdm_get_world_mesh_vertices(h, None, None, 0, 0, None) == INV
    assert L.sdm_world_mesh_device(h, C.byref(p[0]), None, None) == 0 and p[0].value
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert L.sdm_world_mesh_update(shard.h, vp(o)) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_get_world_mesh_info(shard.h, vp(info)) == INV
    assert L.sdm_get_world_mesh_faces(shard.h, None, None, None, 0, 0, C.byref(k64)) == INV
    assert L.sdm_get_world_mesh_vertices(shard.h, None, None, 0, 0, C.byref(k64)) == INV
    assert L.sdm_world_mesh_device(shard.h, None, None, None) == INV
    shard.close()
