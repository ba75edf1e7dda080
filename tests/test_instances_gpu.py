"""The instance table (sdm_instances_update / sdm_get_instances / sdm_get_label_cells) on the GPU against the NumPy
restatement in tests/instances_ref.py: every field of every entry equal (floats by their bit patterns) and all 256 label
counters, under all four flag combinations.  Maps whose result arrays were filled by the real update (a random dense
state then a short drive, and the drive alone; their rings are shifted on two axes), a full-size non-cubic map, the map
shapes of tests/shape_cases.py with crafted patterns, and a fresh map.  Also the snapshot rule in stream order, no side
effects on the map, run-to-run identity and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import instances_ref as ir
from tests import parity_utils as pu
from tests import query_ref as qr
from tests import shape_cases as sc
from tests.dense_state import random_state, stamps_for

pytestmark = pytest.mark.gpu

DRIVE = dict(n_dynamic=2, lateral_extra=(0, 0.5))
MAPS = [("dense", "T0"), ("dense", "C1"), ("driven", "T0"), ("driven", "C1")]
PARAMS = synth.PARAMS["vkitti2"]
_MAPS, _FRAMES, _STRADDLES = {}, {}, []


def _kw(flags):
    return dict(movable_only=bool(flags & ir.MOVABLE_ONLY), observed_only=bool(flags & ir.OBSERVED_ONLY))


def _frames(name):
    if name not in _FRAMES:
        _FRAMES[name] = synth.make_frames(name, 6, **DRIVE)
    return _FRAMES[name]


def get_map(kind, name):
    if (kind, name) not in _MAPS:
        cfg, params, frames = _frames(name)
        g = binding.SdmMap(cfg, params, synth.noise_table())
        if kind == "dense":
            (sx, sy, sz), ring = stamps_for(g)
            g.load_state(random_state(cfg, 41))
            g.set_stamps(sx, sy, sz)
            g.set_ring_state(ring)
        for f in frames:
            g.update(*f)
        g.synchronize()
        _MAPS[kind, name] = (cfg, g)
    cfg, g = _MAPS[kind, name]
    ring = g.ring_state()
    assert sum(e != 0 for e in ring["eq_steps"]) >= 2
    return cfg, g, qr.Geometry(cfg, ring), g.voxels()


def check_all_flags(cfg, g, geo, vox):
    """the table and the label counters under every flag combination -> {flags: table}"""
    tables = {}
    for flags in ir.ALL_FLAGS:
        g.instances_update(**_kw(flags))
        got, origin = g.instances()
        ref = ir.instances(geo, vox, cfg["max_movable_track"], cfg["voxel_size"], flags)
        msg = ir.equal_tables(got, ref)
        assert msg is None, (flags, msg)
        assert np.array_equal(origin.view(np.uint32), ir.origin_of(geo).view(np.uint32))
        assert np.array_equal(g.label_cells(), ir.label_cells(geo, vox, cfg["max_movable_track"], flags)), flags
        assert (got["pad"] == 0).all() and (np.diff(got["track"].astype(np.int64)) > 0).all()
        tables[flags] = got
    return tables


def _movable(cfg, t):
    return (t["track"] >= 1) & (t["track"] <= cfg["max_movable_track"])


@pytest.mark.parametrize("kind,name", MAPS)
def test_table_exact(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    tables = check_all_flags(cfg, g, geo, vox)
    t = tables[0]
    mov = _movable(cfg, t)
    assert np.array_equal(tables[ir.MOVABLE_ONLY]["track"], t["track"][mov])
    if kind == "dense":
        assert len(t) >= 6 and mov.sum() >= 3 and (t["n_guessed"] > 0).any()
        assert (t["mixed_labels"] == 1).any() and (t["mixed_labels"] == 0).any()
    elif name == "T0":
        assert mov.sum() >= 2 and (~mov).sum() >= 2
    else:  # one static track owns everything; the table of the movable ones is empty on a map that is not fresh
        assert len(t) >= 1 and not mov.any() and int(t["n_cells"].sum()) > 100
        assert len(tables[ir.MOVABLE_ONLY]) == 0 and not g.label_cells().any()
    # an instance with counted cells on both sides of the wrap point of a shifted axis: its box in storage order differs
    for e in t:
        lo, hi = ir.storage_box(geo, vox, cfg["max_movable_track"], 0, e["track"])
        for a in range(3):
            n = int(geo.N[a])
            if geo.eq[a] != 0 and lo[a] == 0 and hi[a] == n - 1 and int(e["cell_max"][a]) - int(e["cell_min"][a]) < n - 1:
                assert (int(e["cell_min"][a]), int(e["cell_max"][a])) != (int(lo[a]), int(hi[a]))
                _STRADDLES.append((kind, name, int(e["track"]), a))


def test_some_instance_straddles_the_wrap_point():
    for kind, name in MAPS:   # (fills the list when this test is run on its own; the maps are cached)
        if not _STRADDLES:
            test_table_exact(kind, name)
    assert _STRADDLES


def test_full_size_non_cubic():
    cfg, params, frames = synth.make_frames("REF_VKITTI2", 3)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames:
        g.update(*f)
    g.synchronize()
    geo, vox = qr.Geometry(cfg, g.ring_state()), g.voxels()
    assert tuple(geo.N) == (256, 128, 256)
    tables = check_all_flags(cfg, g, geo, vox)
    assert len(tables[0]) >= 8 and _movable(cfg, tables[0]).sum() >= 3
    g.close()


SHAPE_TRACKS = np.array([3, synth.TRACK_BUILDING, 17], np.uint16)


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_map_shapes(name):
    """crafted patterns on a ring shifted by crafted_steps, brought into the result array by one frame that sees nothing
    (the non-incremental sweep writes every result): x rows of 4, 8 and 16 cells, axes of 512, a 64-voxel map"""
    cfg = sc.config(name)
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    pats = sc.patterns(cfg, ring)
    depth = np.full((cfg["height"], cfg["width"]), np.nan, np.float32)
    cloud = np.zeros(cfg["height"] * cfg["width"], synth.LABELED_POINT)
    cam = np.array(ring["last_pos"], np.float32)
    q = synth.yaw_quat(0.0).astype(np.float32)
    for pattern in ("opposite_corners", "wrap", "tracks", "full_line"):
        cells, unknown, tracks = pats[pattern]
        if tracks is None:
            tracks = SHAPE_TRACKS[np.arange(len(cells)) % 3]
        labels = np.where(tracks <= cfg["max_movable_track"], synth.LABEL_CAR, synth.LABEL_BUILDING).astype(np.uint8)
        g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
        g.load_state(sc.crafted_state(cfg, ring, cells, unknown, tracks, labels))
        g.set_ring_state(ring)
        g.update(depth, cloud, cam, q, None, sync=True)
        got_ring = g.ring_state()
        assert got_ring["eq_steps"] == ring["eq_steps"] and got_ring["map_center"] == ring["map_center"]
        geo, vox = qr.Geometry(cfg, got_ring), g.voxels()
        assert int((vox["occ"] >= 1).sum()) == len(cells), pattern
        tables = check_all_flags(cfg, g, geo, vox)
        t = tables[0]
        assert sorted(t["track"]) == sorted(set(int(x) for x in tracks)) and int(t["n_cells"].sum()) == len(cells), pattern
        assert len(tables[ir.MOVABLE_ONLY]) == len(set(int(x) for x in tracks if x <= cfg["max_movable_track"]))
        g.close()


def test_fresh_map_and_small_cap():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    for flags in ir.ALL_FLAGS:
        g.instances_update(**_kw(flags))
        t, _ = g.instances()
        assert len(t) == 0 and not g.label_cells().any()
        n = C.c_int32(-1)
        assert g.L.sdm_get_instances(g.h, None, 0, C.byref(n), None) == 0 and n.value == 0
    g.close()
    # a cap smaller than the table: the first `cap` entries, the full count, nothing beyond them
    cfg, g, geo, vox = get_map("dense", "T0")
    g.instances_update()
    full, _ = g.instances()
    assert len(full) >= 6
    cap = 3
    buf = np.full((cap + 2) * 144, 0xA5, np.uint8)
    n = C.c_int32(0)
    assert g.L.sdm_get_instances(g.h, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n), None) == 0
    assert n.value == len(full)
    assert np.array_equal(buf[:cap * 144], full[:cap].view(np.uint8)) and (buf[cap * 144:] == 0xA5).all()
    n.value = -1
    assert g.L.sdm_get_instances(g.h, None, 0, C.byref(n), None) == 0 and n.value == len(full)
    small, _ = g.instances(cap=1)    # (the binding asks again with the count it was told)
    assert np.array_equal(small.view(np.uint8), full.view(np.uint8))


def test_snapshot_and_stream_order():
    """Build after frame k, then frames k+1..k+3 (ring shifts) and a clear, nothing synchronised in between: the table is
    frame k's.  A second build with other flags replaces it completely."""
    cfg, params, frames = synth.make_frames("T0", 8, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames[:4]:
        g.update(*f)
    g.synchronize()
    geo_k, vox_k = qr.Geometry(cfg, g.ring_state()), g.voxels()
    g.instances_update()
    for f in frames[4:7]:
        g.update(*f)
    g.clear()
    got, origin = g.instances()
    ref = ir.instances(geo_k, vox_k, cfg["max_movable_track"], cfg["voxel_size"], 0)
    assert len(ref) >= 3
    assert ir.equal_tables(got, ref) is None, ir.equal_tables(got, ref)
    assert np.array_equal(origin, ir.origin_of(geo_k))
    assert np.array_equal(g.label_cells(), ir.label_cells(geo_k, vox_k, cfg["max_movable_track"], 0))
    g.close()
    # a rebuild under other flags holds nothing of the first one's sums, and a third build is the first again
    cfg, g, geo, vox = get_map("dense", "T0")
    first = None
    for flags in (0, ir.MOVABLE_ONLY | ir.OBSERVED_ONLY, 0):
        g.instances_update(**_kw(flags))
        got, _ = g.instances()
        msg = ir.equal_tables(got, ir.instances(geo, vox, cfg["max_movable_track"], cfg["voxel_size"], flags))
        assert msg is None, (flags, msg)
        assert np.array_equal(g.label_cells(), ir.label_cells(geo, vox, cfg["max_movable_track"], flags))
        if first is None:
            first = got
    assert np.array_equal(got.view(np.uint8), first.view(np.uint8))


def test_instances_leave_the_map_alone():
    cfg, params, frames = synth.make_frames("T0", 6, n_dynamic=2)
    a = binding.SdmMap(cfg, params, synth.noise_table())
    b = binding.SdmMap(cfg, params, synth.noise_table())
    for i, f in enumerate(frames):
        a.update(*f)
        b.update(*f)
        b.instances_update(movable_only=bool(i & 1), observed_only=bool(i & 2))
        b.instances()
        b.label_cells()
    a.synchronize()
    b.synchronize()
    rep = pu.compare_maps(a, b, a.S, check_results=True)
    assert not rep, "\n".join(rep)
    assert np.array_equal(a.voxels().view(np.uint64), b.voxels().view(np.uint64))
    sa, sb = a.stats(count_live=True), b.stats(count_live=True)
    for k in sa:
        if k not in ("stage_ms", "host_enqueue_us"):
            assert sa[k] == sb[k], k
    a.close()
    b.close()


def test_run_to_run():
    cfg, g, geo, vox = get_map("dense", "C1")
    runs = []
    for _ in range(2):
        g.instances_update()
        t, _ = g.instances()
        runs.append((t.tobytes(), g.label_cells().tobytes()))
    assert runs[0] == runs[1] and len(runs[0][0]) >= 6 * 144


def test_argument_errors():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    L, INV = g.L, 1
    out = np.zeros(4, binding.INSTANCE)
    lab = np.zeros(256, np.uint32)
    n = C.c_int32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    # before any build
    assert L.sdm_get_instances(g.h, vp(out), 4, C.byref(n), None) == INV
    assert "sdm_instances_update" in L.sdm_last_error().decode()
    assert L.sdm_get_label_cells(g.h, vp(lab)) == INV
    assert "sdm_instances_update" in L.sdm_last_error().decode()
    with pytest.raises(binding.SdmError):
        g.instances()
    with pytest.raises(binding.SdmError):
        g.label_cells()
    assert L.sdm_instances_update(None, 0) == INV
    assert L.sdm_instances_update(g.h, 0x4) == INV
    assert L.sdm_instances_update(g.h, 0x80000000) == INV
    assert L.sdm_instances_update(g.h, 0x3) == 0
    assert L.sdm_get_instances(None, vp(out), 4, C.byref(n), None) == INV
    assert L.sdm_get_instances(g.h, vp(out), -1, C.byref(n), None) == INV
    assert L.sdm_get_instances(g.h, vp(out), 4, None, None) == INV
    assert L.sdm_get_instances(g.h, None, 4, C.byref(n), None) == INV
    assert L.sdm_get_instances(g.h, None, 0, C.byref(n), None) == 0
    assert L.sdm_get_instances(g.h, vp(out), 4, C.byref(n), None) == 0 and n.value == 0
    assert L.sdm_get_label_cells(None, vp(lab)) == INV
    assert L.sdm_get_label_cells(g.h, None) == INV
    assert L.sdm_get_label_cells(g.h, vp(lab)) == 0
    g.close()
    s = binding.SdmMap(cfg, PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert s.L.sdm_instances_update(s.h, 0) == INV
    assert "shard" in s.L.sdm_last_error().decode()
    assert s.L.sdm_get_instances(s.h, vp(out), 4, C.byref(n), None) == INV
    assert s.L.sdm_get_label_cells(s.h, vp(lab)) == INV
    with pytest.raises(binding.SdmError):
        s.instances_update()
    s.close()
