"""The frontiers (sdm_frontiers_update / sdm_get_frontier_clusters / sdm_get_frontier_cells) on the GPU against the NumPy
restatement in tests/frontiers_ref.py: every integer field of every cluster equal, every float field equal by its bit
pattern, and the cell list, the per-cell cluster indices and unknown_faces equal, under both connectivities and
min_cells 1 and 3.  Crafted patterns on the map shapes of tests/shape_cases.py (rings shifted on every axis), maps whose
result arrays were filled by the real update, a full-size non-cubic map; the capacity rule, empty results, the snapshot
rule in stream order, no side effects on the map, run-to-run identity and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import frontiers_ref as fr
from tests import instances_ref as ir
from tests import parity_utils as pu
from tests import query_ref as qr
from tests import shape_cases as sc
from tests.test_instances_gpu import DRIVE, MAPS, get_map

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
COMBOS = [(face, min_cells) for face in (False, True) for min_cells in (1, 3)]
NONE = fr.FRONTIER_NO_CLUSTER
_STRADDLES = []


def check_all(cfg, g, geo, vox, max_cells=None):
    """table, cell list, cluster indices and unknown_faces under every combination -> {(face, min_cells): (table, cells)}.
    max_cells: by default the map's cells (the default capacity, V / 16, is for the thin surfaces of a real map: a
    crafted plane through a map of 64 cells, or a randomly filled one, has more)"""
    occ = fr.occ_grid(geo, vox)
    max_cells = occ.size if max_cells is None else max_cells
    out = {}
    for face, min_cells in COMBOS:
        g.frontiers_update(face_connected=face, min_cells=min_cells, max_cells=max_cells)
        table, origin = g.frontiers()
        cells = g.frontier_cells()
        ref = fr.frontiers_of_block(occ, fr.origin_of(geo), cfg["voxel_size"], face, min_cells)
        msg = fr.equal_all(table, cells, ref)
        assert msg is None, (face, min_cells, msg)
        assert np.array_equal(origin.view(np.uint32), fr.origin_of(geo).view(np.uint32))
        assert (table["pad0"] == 0).all() and (table["pad1"] == 0).all() and (np.diff(table["first_cell"].astype(np.int64)) > 0).all()
        assert (table["n_cells"] >= min_cells).all()
        out[face, min_cells] = (table, cells)
    return out


def straddles(geo, table, cells):
    """(cluster, axis): clusters with cells on both storage ends of a shifted axis that do not span the axis in map cells"""
    cell, cluster, _ = cells
    r = fr.storage_coords(geo, cell)
    found = []
    for a in range(3):
        n = int(geo.N[a])
        if geo.eq[a] == 0:
            continue
        lo = np.unique(cluster[(r[:, a] == 0) & (cluster != NONE)])
        hi = np.unique(cluster[(r[:, a] == n - 1) & (cluster != NONE)])
        for j in np.intersect1d(lo, hi):
            if int(table["cell_max"][j][a]) - int(table["cell_min"][j][a]) < n - 1:
                found.append((int(j), a))
    return found


# ---- crafted patterns on every map shape ------------------------------------------------------------------------------
def _dims(cfg):
    return np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.int64)


def _grid_cells(mask_zyx):
    """(x, y, z) rows of the set cells of a [z, y, x] bool array"""
    z, y, x = np.nonzero(mask_zyx)
    return np.stack([x, y, z], axis=1)


def _face_neighbours(c):
    return np.array([c + d for d in np.vstack([np.eye(3, dtype=np.int64), -np.eye(3, dtype=np.int64)])])


def snake_cells(N):
    """a one-cell-wide serpentine through the plane of the two longest axes, the third axis at its middle: full rows on
    even lines, one connector on odd lines at alternating ends -> (x, y, z) rows"""
    order = np.argsort(-N, kind="stable")
    a, b, c = int(order[0]), int(order[1]), int(order[2])
    rows = []
    for j in range(int(N[b])):
        along = np.arange(N[a]) if j % 2 == 0 else np.array([N[a] - 1 if j % 4 == 1 else 0])
        cell = np.zeros((len(along), 3), np.int64)
        cell[:, a], cell[:, b], cell[:, c] = along, j, N[c] // 2
        rows.append(cell)
    return np.concatenate(rows)


def random_block(N, seed):
    """-> occ [z, y, x]: cells drawn free / unknown / occupied with probability 0.5 / 0.3 / 0.2 over the first
    min(N, 32) cells of every axis (the whole block where no axis is longer), the rest free"""
    sub = np.minimum(N, 32)
    occ = np.zeros(tuple(N[::-1]), np.int8)
    draw = np.random.default_rng(seed).choice(np.array([0, -1, 1], np.int8), size=tuple(sub[::-1]), p=[0.5, 0.3, 0.2])
    occ[:sub[2], :sub[1], :sub[0]] = draw
    return occ


def pattern_block(name, pattern):
    """-> occ [z, y, x] the pattern asks for"""
    N = _dims(sc.config(name))
    occ = np.zeros(tuple(N[::-1]), np.int8)
    if pattern == "slab":
        occ[N[2] // 2:] = -1
    elif pattern == "single":
        occ[N[2] // 2, N[1] // 2, N[0] // 2] = -1
        occ[0, 0, 0] = -1
    elif pattern == "enclosed":
        c = N // 2
        occ[c[2], c[1], c[0]] = -1
        for q in _face_neighbours(c):
            occ[q[2], q[1], q[0]] = 1
    elif pattern == "snake":
        occ[:] = -1
        s = snake_cells(N)
        occ[s[:, 2], s[:, 1], s[:, 0]] = 0
    elif pattern == "random":
        occ = random_block(N, 11 + ord(name))
    return occ


def crafted_map(name, occ):
    """a map of shape `name` on a ring shifted on every axis whose result array reads `occ`: the state is loaded, one
    frame that sees nothing writes every result (as tests/test_instances_gpu.py::test_map_shapes does)"""
    cfg = sc.config(name)
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    g.load_state(sc.crafted_state(cfg, ring, _grid_cells(occ == 1), _grid_cells(occ == -1)))
    g.set_ring_state(ring)
    depth = np.full((cfg["height"], cfg["width"]), np.nan, np.float32)
    cloud = np.zeros(cfg["height"] * cfg["width"], synth.LABELED_POINT)
    g.update(depth, cloud, np.array(ring["last_pos"], np.float32), synth.yaw_quat(0.0).astype(np.float32), None, sync=True)
    got_ring = g.ring_state()
    assert got_ring["eq_steps"] == ring["eq_steps"] and got_ring["map_center"] == ring["map_center"]
    geo, vox = qr.Geometry(cfg, got_ring), g.voxels()
    assert all(e != 0 for e in geo.eq)
    got = fr.occ_grid(geo, vox)
    assert np.array_equal(np.minimum(got, 1), occ)   # (an obstacle reads 1 or 2)
    return cfg, g, geo, vox


@pytest.mark.parametrize("pattern", ["slab", "single", "enclosed", "snake", "random"])
@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_map_shapes(name, pattern):
    occ = pattern_block(name, pattern)
    cfg, g, geo, vox = crafted_map(name, occ)
    N = geo.N
    V = int(N.prod())
    res = check_all(cfg, g, geo, vox, max_cells=V)
    for (face, min_cells), (t, (cell, cluster, faces)) in res.items():
        if pattern == "slab":   # one plane below the unknown half-space, one cluster under either connectivity
            assert len(cell) == N[0] * N[1] and len(t) == 1 and t["n_cells"][0] == N[0] * N[1] and (faces == 1).all()
            assert tuple(t["cell_min"][0]) == (0, 0, N[2] // 2 - 1) and tuple(t["cell_max"][0]) == (N[0] - 1, N[1] - 1, N[2] // 2 - 1)
            r = fr.storage_coords(geo, cell)
            for a in (0, 1):   # its cells lie on both sides of the storage wrap point: storage 0 follows storage N - 1 inside the map
                m = (cell.astype(np.int64) >> (0 if a == 0 else cfg["x_n"])) & (N[a] - 1)
                last, first = m[r[:, a] == N[a] - 1], m[r[:, a] == 0]
                assert len(last) and len(first) and first[0] == last[0] + 1
        elif pattern == "single":   # six cells round the interior cell, three round the corner: outside the map is not unknown
            assert len(cell) == 9 and (faces == 1).all()
            if face:
                assert len(t) == (9 if min_cells == 1 else 0) and (min_cells == 1 or (cluster == NONE).all())
            else:
                assert sorted(t["n_cells"]) == [3, 6] and t["first_cell"][0] == 1 and (cluster != NONE).all()
        elif pattern == "enclosed":
            assert len(cell) == 0 and len(t) == 0
        elif pattern == "snake":   # every free cell, one cluster, its root at the snake's first cell
            n_free = int((occ == 0).sum())
            assert len(cell) == n_free and len(t) == 1 and t["n_cells"][0] == n_free and (cluster == 0).all()
            assert t["first_cell"][0] == cell[0] and t["first_index"][0] == 0 and (faces >= 2).all()
            s = snake_cells(N)[0]
            assert t["first_cell"][0] == s[0] | (s[1] << cfg["x_n"]) | (s[2] << (cfg["x_n"] + cfg["y_n"]))
    if pattern == "random":
        t6, _ = res[True, 1]
        t26, _ = res[False, 1]
        # (A has 64 cells; the others draw 4096 to 32768, of which some 4 % end as a 6-connected cluster)
        assert len(t6) >= (3 if name == "A" else 50) and len(t26) >= 1
        assert (t6["n_cells"] >= 3).any() and (t6["n_cells"] == 1).any()
    g.close()


# ---- real maps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", MAPS)
def test_real_maps(kind, name):
    cfg, g, geo, vox = get_map(kind, name)
    res = check_all(cfg, g, geo, vox)
    for key, (t, cells) in res.items():
        print(kind, name, "face_connected, min_cells", key, ":", len(cells[0]), "cells,", len(t), "clusters")
        _STRADDLES.extend((kind, name, key) + s for s in straddles(geo, t, cells))
    # More than one cluster: under 6-connectivity, every cluster kept.  The free space of a driven map is what a few
    # frusta swept, and its border with the unknown can be one 26-connected surface (it is on the driven T0 map: 566
    # cells, one cluster, equal to the restatement); face steps alone do not get along a slanted surface.
    assert len(res[True, 1][0]) > 1


def test_some_cluster_spans_the_wrap_point():
    for kind, name in MAPS:   # (fills the list when this test is run on its own; the maps are cached)
        if not _STRADDLES:
            test_real_maps(kind, name)
    assert _STRADDLES


def test_full_size_non_cubic():
    cfg, params, frames = synth.make_frames("REF_VKITTI2", 3)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames:
        g.update(*f)
    g.synchronize()
    geo, vox = qr.Geometry(cfg, g.ring_state()), g.voxels()
    assert tuple(geo.N) == (256, 128, 256)
    res = check_all(cfg, g, geo, vox, max_cells=0)   # the default capacity: V / 16
    t, _ = res[False, 1]
    assert len(t) > 1 and int(t["n_cells"].sum()) > 1000
    # a longer cell list and the default one again: the flag scan runs over capacity + 1 entries and changes between the
    # one-launch and the two-launch form of exclusive_scan_u32 on the way
    want = (g.frontiers()[0].tobytes(),) + tuple(x.tobytes() for x in g.frontier_cells())   # (True, 3), the last combination
    for max_cells in (g.V // 4, 0, g.V // 4, 0):
        g.frontiers_update(face_connected=True, min_cells=3, max_cells=max_cells)
        assert (g.frontiers()[0].tobytes(),) + tuple(x.tobytes() for x in g.frontier_cells()) == want, max_cells
    g.close()


# ---- capacity, empty results, snapshot, side effects, run to run, arguments ------------------------------------------
def _raw_cells(g, n_alloc):
    cell, cluster, faces = np.full(n_alloc, 0xA5A5A5A5, np.uint32), np.full(n_alloc, 0xA5A5A5A5, np.uint32), np.full(n_alloc, 0xA5, np.uint8)
    n = C.c_int64(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = g.L.sdm_get_frontier_cells(g.h, vp(cell), vp(cluster), vp(faces), n_alloc, C.byref(n))
    return rc, n.value, cell, cluster, faces


def test_capacity():
    occ = pattern_block("B", "random")
    cfg, g, geo, vox = crafted_map("B", occ)
    ref = fr.frontiers(geo, vox, cfg["voxel_size"])
    true_n = len(ref["cell"])
    assert true_n > 1000
    CAPACITY = 4
    g.frontiers_update(max_cells=true_n // 2)
    out, n = np.zeros(4, binding.FRONTIER_CLUSTER), C.c_int32(0)
    assert g.L.sdm_get_frontier_clusters(g.h, out.ctypes.data_as(C.c_void_p), 4, C.byref(n), None) == CAPACITY
    assert "max_cells" in g.L.sdm_last_error().decode()
    rc, n_cells, cell, cluster, faces = _raw_cells(g, true_n)
    assert rc == CAPACITY and n_cells == true_n
    assert (cell == 0xA5A5A5A5).all() and (cluster == 0xA5A5A5A5).all() and (faces == 0xA5).all()   # nothing truncated
    with pytest.raises(binding.SdmError):
        g.frontiers()
    for face, min_cells in COMBOS:   # a list of exactly the count: the build before it left nothing behind
        g.frontiers_update(face_connected=face, min_cells=min_cells, max_cells=true_n)
        want = fr.frontiers(geo, vox, cfg["voxel_size"], face, min_cells)
        msg = fr.equal_all(g.frontiers()[0], g.frontier_cells(), want)
        assert msg is None, (face, min_cells, msg)
    g.frontiers_update(max_cells=true_n - 1)   # one short, on memory that is long enough
    assert _raw_cells(g, true_n)[:2] == (CAPACITY, true_n)
    g.frontiers_update(max_cells=1 << 40)   # (more than the map has cells: the whole map's worth)
    assert fr.equal_all(g.frontiers()[0], g.frontier_cells(), ref) is None
    # a cell getter with a short cap: the first cells, the count, nothing beyond
    rc, n_cells, cell, cluster, faces = _raw_cells(g, 10)
    assert rc == 0 and n_cells == true_n and np.array_equal(cell, ref["cell"][:10])
    n64 = C.c_int64(0)
    assert g.L.sdm_get_frontier_cells(g.h, None, None, None, 0, C.byref(n64)) == 0 and n64.value == true_n
    g.close()


def test_fresh_map_and_map_without_unknown():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())   # fresh: every cell unknown, none free
    cfg_a, h, geo, vox = crafted_map("B", np.zeros((64, 32, 4), np.int8))   # every cell free, none unknown
    assert not (vox["occ"] == -1).any()
    for m in (g, h):
        for face, min_cells in COMBOS:
            m.frontiers_update(face_connected=face, min_cells=min_cells)
            t, _ = m.frontiers()
            cell, cluster, faces = m.frontier_cells()
            assert len(t) == 0 and len(cell) == 0 and len(cluster) == 0 and len(faces) == 0
            n = C.c_int32(-1)
            assert m.L.sdm_get_frontier_clusters(m.h, None, 0, C.byref(n), None) == 0 and n.value == 0
        m.close()


def test_snapshot_and_stream_order():
    """Build after frame k, then two more frames (ring shifts) and a clear, nothing synchronised in between: the answer
    is frame k's.  A new build gives the new one."""
    cfg, params, frames = synth.make_frames("T0", 8, **DRIVE)
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames[:4]:
        g.update(*f)
    g.synchronize()
    geo_k, vox_k = qr.Geometry(cfg, g.ring_state()), g.voxels()
    g.frontiers_update(max_cells=g.V)
    for f in frames[4:6]:
        g.update(*f)
    g.clear()
    table, origin = g.frontiers()
    ref = fr.frontiers(geo_k, vox_k, cfg["voxel_size"])
    assert len(ref["table"]) >= 1 and len(ref["cell"]) > 100
    msg = fr.equal_all(table, g.frontier_cells(), ref)
    assert msg is None, msg
    assert np.array_equal(origin, fr.origin_of(geo_k))
    g.update(*frames[6])
    g.synchronize()
    geo_n, vox_n = qr.Geometry(cfg, g.ring_state()), g.voxels()
    g.frontiers_update(face_connected=True, max_cells=g.V)
    new = fr.frontiers(geo_n, vox_n, cfg["voxel_size"], True)
    assert not np.array_equal(new["cell"], ref["cell"])
    msg = fr.equal_all(g.frontiers()[0], g.frontier_cells(), new)
    assert msg is None, msg
    g.close()


def test_frontiers_leave_the_map_alone():
    cfg, params, frames = synth.make_frames("T0", 6, n_dynamic=2)
    a = binding.SdmMap(cfg, params, synth.noise_table())
    b = binding.SdmMap(cfg, params, synth.noise_table())
    for i, f in enumerate(frames):
        a.update(*f)
        b.update(*f)
        b.frontiers_update(face_connected=bool(i & 1), min_cells=1 + (i & 2), max_cells=b.V)
        b.frontiers()
        b.frontier_cells()
    a.synchronize()
    b.synchronize()
    rep = pu.compare_maps(a, b, a.S, check_results=True)
    assert not rep, "\n".join(rep)
    assert np.array_equal(a.voxels().view(np.uint64), b.voxels().view(np.uint64))
    for m in (a, b):
        m.esdf_update()
        m.instances_update()
    for x, y in zip(a.esdf()[:2], b.esdf()[:2]):
        assert np.array_equal(x, y)
    assert ir.equal_tables(a.instances()[0], b.instances()[0]) is None
    a.close()
    b.close()


def test_run_to_run():
    cfg, g, geo, vox = get_map("dense", "C1")
    runs = []
    for _ in range(2):
        g.frontiers_update(max_cells=g.V)
        t, _ = g.frontiers()
        runs.append((t.tobytes(),) + tuple(x.tobytes() for x in g.frontier_cells()))
    assert runs[0] == runs[1] and len(runs[0][0]) >= 2 * 96


def test_argument_errors():
    cfg = synth.CONFIGS["T0"]
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    L, INV = g.L, 1
    out = np.zeros(4, binding.FRONTIER_CLUSTER)
    cell = np.zeros(4, np.uint32)
    n, n64 = C.c_int32(0), C.c_int64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    # before any build
    assert L.sdm_get_frontier_clusters(g.h, vp(out), 4, C.byref(n), None) == INV
    assert "sdm_frontiers_update" in L.sdm_last_error().decode()
    assert L.sdm_get_frontier_cells(g.h, vp(cell), None, None, 4, C.byref(n64)) == INV
    assert "sdm_frontiers_update" in L.sdm_last_error().decode()
    with pytest.raises(binding.SdmError):
        g.frontiers()
    with pytest.raises(binding.SdmError):
        g.frontier_cells()
    assert L.sdm_frontiers_update(None, 0, 1, 0) == INV
    assert L.sdm_frontiers_update(g.h, 0x2, 1, 0) == INV
    assert L.sdm_frontiers_update(g.h, 0x80000000, 1, 0) == INV
    assert L.sdm_frontiers_update(g.h, 0, 1, -1) == INV
    assert L.sdm_frontiers_update(g.h, 0x1, -5, 0) == 0
    assert L.sdm_get_frontier_clusters(None, vp(out), 4, C.byref(n), None) == INV
    assert L.sdm_get_frontier_clusters(g.h, vp(out), -1, C.byref(n), None) == INV
    assert L.sdm_get_frontier_clusters(g.h, vp(out), 4, None, None) == INV
    assert L.sdm_get_frontier_clusters(g.h, None, 4, C.byref(n), None) == INV
    assert L.sdm_get_frontier_clusters(g.h, None, 0, C.byref(n), None) == 0
    assert L.sdm_get_frontier_clusters(g.h, vp(out), 4, C.byref(n), None) == 0 and n.value == 0
    assert L.sdm_get_frontier_cells(None, vp(cell), None, None, 4, C.byref(n64)) == INV
    assert L.sdm_get_frontier_cells(g.h, vp(cell), None, None, -1, C.byref(n64)) == INV
    assert L.sdm_get_frontier_cells(g.h, vp(cell), None, None, 4, None) == INV
    assert L.sdm_get_frontier_cells(g.h, None, None, None, 4, C.byref(n64)) == 0 and n64.value == 0
    g.close()
    s = binding.SdmMap(cfg, PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert s.L.sdm_frontiers_update(s.h, 0, 1, 0) == INV
    assert "shard" in s.L.sdm_last_error().decode()
    assert s.L.sdm_get_frontier_clusters(s.h, vp(out), 4, C.byref(n), None) == INV
    assert s.L.sdm_get_frontier_cells(s.h, vp(cell), None, None, 4, C.byref(n64)) == INV
    with pytest.raises(binding.SdmError):
        s.frontiers_update()
    s.close()
