"""The surface mesh (include/sdm.h: sdm_mesh_update / sdm_get_mesh_info / sdm_get_mesh_faces / sdm_get_mesh_vertices /
sdm_mesh_device) against tests/mesh_ref.py, bit for bit: faces, quads, corners, xyz, the info block, the origin.

Crafted maps on every shape of tests/shape_cases.py with the ring shifted on every axis, the patterns of shape_cases, full,
empty and checkerboard blocks, every legal flag combination, label masks and tracks; the filled maps of
tests/test_instances_gpu.py; the capacity rule; a second build; the snapshot rule; no side effects; the device pointers;
the argument checks."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import esdf_ref as er
from tests import mesh_ref as mr
from tests import parity_utils as pu
from tests import query_ref as qr
from tests import shape_cases as sc
from tests.test_ground_gpu import crafted_map, random_block
from tests.test_instances_gpu import DRIVE, MAPS, get_map

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
ROAD, BUILDING, CAR = synth.LABEL_ROAD, synth.LABEL_BUILDING, synth.LABEL_CAR
CAPACITY, INV = 4, 1
NAMES = ("faces", "quads", "corners", "xyz")
FLAG_SETS = [s | o | u | b for s in (0, mr.STATIC_ONLY, mr.MOVABLE_ONLY) for o in (0, mr.OBSERVED_ONLY)
             for u in (0, mr.SKIP_UNKNOWN_FACES) for b in (0, mr.SKIP_BORDER_FACES)]   # every legal combination, each flag alone among them


def origin_of(geo):
    return (geo.center + geo.pmin).astype(np.float32)


def reference(cfg, geo, snap, opt, fit=False):
    return mr.build(snap, cfg["max_movable_track"], opt, cfg["voxel_size"], origin_of(geo), fit)


def compare(got, ref, geo, opt):
    for name in NAMES:
        assert got[name].shape == ref[name].shape, (opt, name, got[name].shape, ref[name].shape)
        if got[name].tobytes() != ref[name].tobytes():
            a, b = got[name].reshape(len(got[name]), -1), ref[name].reshape(len(ref[name]), -1)
            bad = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(a, b)])
            raise AssertionError((opt, name, len(bad), bad[:4].tolist(), got[name][bad[:2]], ref[name][bad[:2]]))
    assert got["info"].tobytes() == ref["info"].tobytes(), (opt, got["info"], ref["info"])
    assert got["origin"].tobytes() == origin_of(geo).tobytes()


def raw_lists(g, n_faces, n_vertices, canary=3):
    """both list getters called directly, the caller's buffers `canary` entries longer than the caps given ->
    (rc, n_out, the buffers) of each"""
    faces, quads = np.full(n_faces + canary, 0xA5, np.uint8).repeat(12).view(binding.MESH_FACE), np.full((n_faces + canary, 4), 0xA5A5A5A5, np.uint32)
    corners, xyz = np.full((n_vertices + canary) * 8, 0xA5, np.uint8).view(binding.MESH_VERTEX), np.full((n_vertices + canary, 3), -7.0, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nf, nv = C.c_int64(-1), C.c_int64(-1)
    rc_f = g.L.sdm_get_mesh_faces(g.h, vp(faces), vp(quads), n_faces, C.byref(nf))
    rc_v = g.L.sdm_get_mesh_vertices(g.h, vp(corners), vp(xyz), n_vertices, C.byref(nv))
    return (rc_f, nf.value, faces, quads), (rc_v, nv.value, corners, xyz)


def untouched(buffers, start):
    return all((b[start:].view(np.uint8) == 0xA5).all() if b.dtype != np.float32 else (b[start:] == -7.0).all() for b in buffers)


def check_build(cfg, g, geo, snap, opt, fit=True):
    """one build against the restatement -> the reference.  fit: ask for exactly the lists the mesh needs (a capacity of 0
    would mean the default); otherwise the options' capacities stand, and a build over them is checked as such."""
    ref = reference(cfg, geo, snap, opt, fit)
    opt = ref["opt"]
    g.mesh_update(**mr.update_kwargs(opt))
    info, origin = g.mesh_info()
    assert info.tobytes() == ref["info"].tobytes(), (opt, info, ref["info"])
    if ref["over"]:
        nf, nv = int(ref["info"]["n_faces"]), int(ref["info"]["n_vertices"])
        (rc_f, n_f, *fb), (rc_v, n_v, *vb) = raw_lists(g, nf, nv)
        assert (rc_f, n_f, rc_v, n_v) == (CAPACITY, nf, CAPACITY, nv) and "sdm_mesh_update" in g.L.sdm_last_error().decode()
        assert untouched(fb, 0) and untouched(vb, 0)           # no list entry of a build over capacity
        with pytest.raises(binding.SdmError):
            g.mesh()
    else:
        assert not fit or (info["n_faces"] == max(len(ref["faces"]), 0) and info["options"]["max_faces"] >= info["n_faces"])
        compare(g.mesh(), ref, geo, opt)
    return ref


class Seen:
    """what a run has met: a test that never meets a case must fail, not pass"""
    def __init__(self):
        self.dir, self.kind, self.skipped = np.zeros(6, np.int64), np.zeros(4, np.int64), np.zeros(2, np.int64)
        self.plain = {}

    def add(self, ref, opt):
        self.dir += ref["info"]["faces_by_dir"]
        self.kind += ref["info"]["faces_by_kind"]
        key = (opt["flags"] & ~(mr.SKIP_UNKNOWN_FACES | mr.SKIP_BORDER_FACES), opt["track"], None if opt["labels"] is None else tuple(opt["labels"]))
        if not opt["flags"] & (mr.SKIP_UNKNOWN_FACES | mr.SKIP_BORDER_FACES):
            self.plain[key] = ref["info"]["faces_by_kind"].astype(np.int64)
        elif key in self.plain:                                 # the same solid cells without the skip flags: what is missing now
            by_kind = self.plain[key]
            gone = by_kind.sum() - int(ref["info"]["n_faces"])
            u, b = bool(opt["flags"] & mr.SKIP_UNKNOWN_FACES), bool(opt["flags"] & mr.SKIP_BORDER_FACES)
            assert gone == u * by_kind[1] + b * by_kind[2], (opt, gone, by_kind)
            self.skipped += [u * by_kind[1], b * by_kind[2]]

    def check(self):
        assert (self.dir > 0).all() and (self.kind > 0).all() and (self.skipped > 0).all(), (self.dir, self.kind, self.skipped)


def option_sets(big):
    two = [mr.options(labels=[ROAD, CAR]), mr.options(labels=[ROAD, CAR], flags=mr.SKIP_UNKNOWN_FACES | mr.SKIP_BORDER_FACES)]
    if big:
        return two
    return ([mr.options(flags=f) for f in FLAG_SETS] + two +
            [mr.options(labels=[BUILDING], flags=mr.SKIP_BORDER_FACES), mr.options(track=3), mr.options(track=synth.TRACK_BUILDING),
             mr.options(track=4444), mr.options(labels=[]), mr.options(track=5, labels=[ROAD, BUILDING], flags=mr.MOVABLE_ONLY),
             mr.options(track=5, flags=mr.STATIC_ONLY)])


# ---- crafted maps: every shape ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_random_blocks_on_every_shape(name):
    cfg = sc.config(name)
    g, geo, snap = crafted_map(cfg, *random_block(cfg, 50 + ord(name)))
    seen = Seen()
    for opt in option_sets(big=name in "DEF"):
        ref = check_build(cfg, g, geo, snap, opt)
        assert not ref["over"]
        seen.add(ref, opt)
        if opt["labels"] == [] or opt["track"] == 4444:
            assert ref["info"]["n_faces"] == 0 and ref["info"]["n_solid"] == 0
    seen.check()
    g.close()


def block_of(cfg, occupied=(), unknown=(), tracks=None):
    N = [1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]]
    occ, label, track = (np.zeros(tuple(N[::-1]), dt) for dt in (np.int8, np.uint8, np.uint16))
    occupied, unknown = np.asarray(occupied, np.int64).reshape(-1, 3), np.asarray(unknown, np.int64).reshape(-1, 3)
    occ[unknown[:, 2], unknown[:, 1], unknown[:, 0]] = -1
    occ[occupied[:, 2], occupied[:, 1], occupied[:, 0]] = 1
    label[occ == 1] = BUILDING
    track[occupied[:, 2], occupied[:, 1], occupied[:, 0]] = synth.TRACK_BUILDING if tracks is None else tracks
    return occ, label, track


@pytest.mark.parametrize("name", ["A", "C", "F"])
def test_patterns(name):
    cfg = sc.config(name)
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    V = 1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])
    N = np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.int64)
    for pattern, (occupied, unknown, tracks) in sc.patterns(cfg, ring).items():
        g, geo, snap = crafted_map(cfg, *block_of(cfg, occupied, unknown, tracks))
        for opt in (mr.options(max_faces=6 * V), mr.options(flags=mr.STATIC_ONLY | mr.SKIP_BORDER_FACES, max_faces=6 * V)):
            ref = check_build(cfg, g, geo, snap, opt, fit=False)          # (the largest lists there are)
            assert not ref["over"], pattern
        plain = reference(cfg, geo, snap, mr.options(max_faces=6 * V))["info"]
        if pattern == "corner":
            assert plain["n_faces"] == 6 and plain["n_vertices"] == 8 and plain["faces_by_kind"].tolist() == [3, 0, 3, 0]
        if pattern == "unknown_only":
            assert plain["n_faces"] == 0 and plain["n_vertices"] == 0
        if pattern == "full_line":
            assert plain["n_faces"] == 4 * N.max() + 2 and plain["faces_by_kind"][2] >= 2
        g.close()
    # a full block: the map's hull, all of kind 2; nothing with SKIP_BORDER_FACES.  An empty one: nothing, and the getters say so
    g, geo, snap = crafted_map(cfg, *block_of(cfg, np.argwhere(np.ones(tuple(N), bool))))
    ref = check_build(cfg, g, geo, snap, mr.options(max_faces=6 * V), fit=False)
    assert ref["info"]["n_faces"] == 2 * (N[0] * N[1] + N[1] * N[2] + N[0] * N[2]) and ref["info"]["faces_by_kind"].tolist()[:2] == [0, 0]
    assert ref["info"]["faces_by_kind"][3] == 0 and ref["info"]["n_solid"] == V
    assert check_build(cfg, g, geo, snap, mr.options(flags=mr.SKIP_BORDER_FACES), fit=False)["info"]["n_faces"] == 0
    g.close()
    g, geo, snap = crafted_map(cfg, *block_of(cfg))
    ref = check_build(cfg, g, geo, snap, mr.options(), fit=False)
    assert ref["info"]["n_faces"] == 0 and ref["info"]["n_vertices"] == 0 and ref["info"]["n_solid"] == 0
    (rc_f, n_f, *fb), (rc_v, n_v, *vb) = raw_lists(g, 0, 0)
    assert (rc_f, n_f, rc_v, n_v) == (0, 0, 0, 0) and untouched(fb, 0) and untouched(vb, 0)
    g.close()


def checkerboard(cfg):
    N = [1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]]
    z, y, x = np.indices(tuple(N[::-1]))
    occ = ((x + y + z) & 1).astype(np.int8)
    return occ, np.where(occ == 1, BUILDING, 0).astype(np.uint8), np.where(occ == 1, synth.TRACK_BUILDING, 0).astype(np.uint16)


# ---- the capacity rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_checkerboard_and_the_capacities(name):
    """six faces per solid cell, 3 V faces: beyond the default capacity"""
    cfg = sc.config(name)
    V = 1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])
    g, geo, snap = crafted_map(cfg, *checkerboard(cfg))
    ref = check_build(cfg, g, geo, snap, mr.options(), fit=False)
    nf, nv = int(ref["info"]["n_faces"]), int(ref["info"]["n_vertices"])
    assert ref["over"] and nf == 3 * V and ref["info"]["n_solid"] == V // 2 and ref["info"]["faces_by_dir"].sum() == 0
    n_corners = int(np.prod([(1 << cfg[k]) + 1 for k in ("x_n", "y_n", "z_n")]))
    assert nv == n_corners - 4                                  # all but the four map corners whose only cell is free
    # the true counts, exactly: succeeds
    fits = check_build(cfg, g, geo, snap, mr.options(max_faces=nf, max_vertices=nv), fit=False)
    assert not fits["over"] and fits["info"]["faces_by_dir"].tolist() == [V // 2] * 6
    (rc_f, n_f, faces, quads), (rc_v, n_v, corners, xyz) = raw_lists(g, nf, nv)
    assert (rc_f, n_f, rc_v, n_v) == (0, nf, 0, nv) and untouched((faces, quads), nf) and untouched((corners, xyz), nv)
    assert faces[:nf].tobytes() == fits["faces"].tobytes() and xyz[:nv].tobytes() == fits["xyz"].tobytes()
    # a getter with a short cap: the first entries, the true count, nothing beyond
    (rc_f, n_f, faces, quads), (rc_v, n_v, corners, xyz) = raw_lists(g, 5, 7)
    assert (rc_f, n_f, rc_v, n_v) == (0, nf, 0, nv) and untouched((faces, quads), 5) and untouched((corners, xyz), 7)
    assert quads[:5].tobytes() == fits["quads"][:5].tobytes() and corners[:7].tobytes() == fits["corners"][:7].tobytes()
    # one short of either list: over
    for short in (mr.options(max_faces=nf, max_vertices=nv - 1), mr.options(max_faces=nf - 1, max_vertices=nv)):
        assert check_build(cfg, g, geo, snap, short, fit=False)["over"]
    # only the vertex list too small: faces fit the default of a larger request
    assert check_build(cfg, g, geo, snap, mr.options(max_faces=6 * V, max_vertices=8), fit=False)["over"]
    assert not check_build(cfg, g, geo, snap, mr.options(max_faces=6 * V), fit=False)["over"]
    g.close()


# ---- filled maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", MAPS)
def test_filled_maps(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    snap = er.snapshot_grid(geo, vox)
    for opt in (mr.options(), mr.options(flags=mr.MOVABLE_ONLY)):
        ref = check_build(cfg, g, geo, snap, opt, fit=False)             # the default capacities, over or not
        if ref["over"]:
            ref = check_build(cfg, g, geo, snap, opt)
        assert not ref["over"]
        if kind == "dense" and opt["flags"] == 0:
            assert ref["info"]["n_faces"] > 0 and (ref["info"]["faces_by_dir"] > 0).all()


# ---- a second build, run to run ------------------------------------------------------------------------------------------
def test_a_second_build_sees_nothing_of_the_first():
    cfg = sc.config("B")
    block = random_block(cfg, 77)
    dense, sparse = mr.options(), mr.options(track=3, labels=[CAR], flags=mr.SKIP_UNKNOWN_FACES)
    g, geo, snap = crafted_map(cfg, *block)
    first = check_build(cfg, g, geo, snap, dense)
    ref = check_build(cfg, g, geo, snap, sparse)                          # (a stale corner mask fails here)
    assert 0 < ref["info"]["n_vertices"] < first["info"]["n_vertices"]
    second = g.mesh()
    fresh, geo2, snap2 = crafted_map(cfg, *block)
    assert np.array_equal(snap, snap2)
    check_build(cfg, fresh, geo2, snap2, sparse)
    again = fresh.mesh()
    for name in NAMES + ("info",):
        assert second[name].tobytes() == again[name].tobytes(), name
    runs = []
    for _ in range(2):
        check_build(cfg, g, geo, snap, dense)
        m = g.mesh()
        runs.append(tuple(m[name].tobytes() for name in NAMES + ("info", "origin")))
    assert runs[0] == runs[1]
    g.close()
    fresh.close()


# ---- the snapshot rule, side effects, the device pointers -------------------------------------------------------------------
def test_snapshot_and_stream_order():
    """Build after frame k, then two more frames (ring shifts) and a clear, nothing synchronised in between: the mesh is
    frame k's.  A new build gives the new frame's."""
    cfg, params, frames = synth.make_frames("T0", 8, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames[:4]:
        g.update(*f)
    g.synchronize()
    geo_k = qr.Geometry(cfg, g.ring_state())
    snap_k = er.snapshot_grid(geo_k, g.voxels())
    opt = mr.options(max_faces=6 * g.V)
    g.mesh_update(**mr.update_kwargs(opt))
    for f in frames[4:6]:
        g.update(*f)
    g.clear()
    ref = reference(cfg, geo_k, snap_k, opt)
    assert ref["info"]["n_faces"] > 0
    compare(g.mesh(), ref, geo_k, opt)
    g.update(*frames[6])
    g.synchronize()
    geo_n = qr.Geometry(cfg, g.ring_state())
    new = check_build(cfg, g, geo_n, er.snapshot_grid(geo_n, g.voxels()), opt, fit=False)
    assert new["faces"].tobytes() != ref["faces"].tobytes()
    g.close()


def test_mesh_leaves_the_map_alone():
    cfg, params, frames = synth.make_frames("T0", 6, n_dynamic=2)
    a = binding.SdmMap(cfg, params, synth.noise_table())
    b = binding.SdmMap(cfg, params, synth.noise_table())
    for i, f in enumerate(frames):
        a.update(*f)
        b.update(*f)
        b.mesh_update(static_only=bool(i & 1), skip_unknown_faces=bool(i & 2), max_faces=(6 * b.V if i % 3 else 0))
    a.synchronize()
    b.synchronize()
    rep = pu.compare_maps(a, b, a.S, check_results=True)
    assert not rep, "\n".join(rep)
    assert np.array_equal(a.voxels().view(np.uint64), b.voxels().view(np.uint64))
    for m in (a, b):
        m.frontiers_update()
    assert a.frontiers()[0].tobytes() == b.frontiers()[0].tobytes()
    a.close()
    b.close()


def test_device_pointers():
    cfg = sc.config("C")
    g, geo, snap = crafted_map(cfg, *random_block(cfg, 5))
    ref = check_build(cfg, g, geo, snap, mr.options())
    nf, nv = len(ref["faces"]), len(ref["corners"])
    assert nf > 0
    d_faces, d_quads, d_corners = g.mesh_device()
    g.synchronize()
    assert g.device_download(d_faces, nf * 12, binding.MESH_FACE).tobytes() == ref["faces"].tobytes()
    assert g.device_download(d_quads, nf * 16, np.uint32).tobytes() == ref["quads"].tobytes()
    assert g.device_download(d_corners, nv * 8, binding.MESH_VERTEX).tobytes() == ref["corners"].tobytes()
    g.close()


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    L = g.L
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    info, n = np.zeros(1, binding.MESH_INFO), C.c_int64(0)
    faces, corners = np.zeros(4, binding.MESH_FACE), np.zeros(4, binding.MESH_VERTEX)
    p = [C.c_void_p() for _ in range(3)]
    # before any build
    assert L.sdm_get_mesh_info(g.h, vp(info), None) == INV and "sdm_mesh_update" in L.sdm_last_error().decode()
    assert L.sdm_get_mesh_faces(g.h, vp(faces), None, 4, C.byref(n)) == INV
    assert L.sdm_get_mesh_vertices(g.h, vp(corners), None, 4, C.byref(n)) == INV
    assert L.sdm_mesh_device(g.h, *(C.byref(x) for x in p)) == INV
    for call in (g.mesh, g.mesh_info, g.mesh_device):
        with pytest.raises(binding.SdmError):
            call()

    def update(**kw):
        o = np.zeros(1, binding.MESH_OPTIONS)
        o["track"], o["labels"] = -1, 0xFFFFFFFF
        for k, v in kw.items():
            o[k] = v
        return L.sdm_mesh_update(g.h, vp(o))

    assert L.sdm_mesh_update(g.h, None) == INV
    for bad in (dict(flags=0x20), dict(flags=0x80000000), dict(flags=mr.STATIC_ONLY | mr.MOVABLE_ONLY), dict(track=-2), dict(track=65536),
                dict(max_faces=-1), dict(max_vertices=-1)):
        assert update(**bad) == INV, bad
        assert L.sdm_get_mesh_info(g.h, vp(info), None) == INV              # (a refused build is no build)
    for good in (dict(), dict(flags=0x1D), dict(flags=0x1E), dict(track=0), dict(track=65535), dict(max_faces=1 << 40, max_vertices=1 << 40)):
        assert update(**good) == 0, good
    assert L.sdm_get_mesh_info(g.h, None, None) == 0 and L.sdm_get_mesh_info(g.h, vp(info), None) == 0
    V = g.V
    assert info[0]["n_faces"] == 0 and info[0]["options"]["max_faces"] == 6 * V and info[0]["options"]["max_vertices"] == 33 ** 3   # clamped
    for fn, a in ((L.sdm_get_mesh_faces, faces), (L.sdm_get_mesh_vertices, corners)):
        assert fn(g.h, vp(a), None, -1, C.byref(n)) == INV
        assert fn(g.h, vp(a), None, 4, None) == INV
        assert fn(g.h, None, None, 4, C.byref(n)) == 0 and n.value == 0
        assert fn(g.h, vp(a), None, 0, C.byref(n)) == 0
    assert L.sdm_mesh_device(g.h, None, None, None) == 0 and L.sdm_mesh_device(g.h, *(C.byref(x) for x in p)) == 0 and all(x.value for x in p)
    g.close()
    s = binding.SdmMap(cfg, PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    o = np.zeros(1, binding.MESH_OPTIONS)
    o["track"] = -1
    assert s.L.sdm_mesh_update(s.h, vp(o)) == INV and "shard" in s.L.sdm_last_error().decode()
    assert s.L.sdm_get_mesh_info(s.h, vp(info), None) == INV
    assert s.L.sdm_get_mesh_faces(s.h, vp(faces), None, 4, C.byref(n)) == INV
    assert s.L.sdm_get_mesh_vertices(s.h, vp(corners), None, 4, C.byref(n)) == INV
    assert s.L.sdm_mesh_device(s.h, *(C.byref(x) for x in p)) == INV
    with pytest.raises(binding.SdmError):
        s.mesh_update()
    s.close()
