"""The map shapes of tests/shape_cases.py on the GPU: maps of 64 voxels, x rows of 4 and 8 cells, a y axis of 4 cells,
axes of 512 cells on non-cubic maps, and the shipped ZED2 grid.  Against the oracle bit for bit (free-running frames,
non-incremental sweeps of a random dense state, the emitted clouds in full), and the queries and the distance field
against tests/query_ref.py and tests/esdf_ref.py, on frame-filled maps and on crafted occupancy patterns on a shifted
ring.  Also queries of more than one 2^20-item chunk, in host and device mode."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import esdf_ref as er
from tests import parity_utils as pu
from tests import query_ref as qr
from tests import shape_cases as sc
from tests.dense_state import random_state, stamps_for
from tests.test_esdf_gpu import FLAGS, _check_query, _flag_kw, _query_points
from tests.test_queries_gpu import _check_segments, _hand_segments, _span

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
N_FRAMES = 24
_DRIVEN = {}


def _driven(name):
    """both implementations through N_FRAMES free-running frames, compared every 6th; -> cfg, o, g, reports, per-frame
    ring offsets and occupied counts, the last camera position"""
    if name not in _DRIVEN:
        cfg = sc.config(name)
        o, g = pu.make_pair(cfg, PARAMS, synth.noise_table())
        S = 1 << cfg["p_n"]
        reps, eqs, n_occ, pos = [], [], [], None
        for t, depth, cloud, pos, q, mv, remove in sc.drive(name, PARAMS, N_FRAMES, seed=17):
            o.update(depth, cloud, pos, q, mv, remove)
            g.update(depth, cloud, pos, q, mv, remove)
            eqs.append(o.ring_state()["eq_steps"])
            if t % 6 == 5:
                g.synchronize()
                reps += pu.compare_maps(o, g, S, check_results=True, check_bins=True, tag="%s frame %d: " % (name, t))
            n_occ.append(int((o.voxels()["occ"] > 0).sum()))
        g.synchronize()
        _DRIVEN[name] = (cfg, o, g, reps, np.array(eqs), n_occ, pos)
    return _DRIVEN[name]


def _min_occupied(name):
    return 4 if name == "A" else 200     # (case A has 64 voxels)


@pytest.mark.parametrize("name", sc.PARITY_CASES)
def test_free_running_frames(name):
    cfg, o, g, reps, eqs, n_occ, _ = _driven(name)
    assert not reps, "\n".join(reps)
    assert (eqs != 0).any(axis=0).all(), "the ring never moved on some axis"
    assert (np.diff(eqs, axis=0) > 0).any(axis=0).all() and (np.diff(eqs, axis=0) < 0).any(axis=0).all()
    assert max(n_occ) >= _min_occupied(name), n_occ
    vo = o.voxels()
    assert (vo["occ"] == 0).any() and (vo["occ"] < 0).any()
    assert np.array_equal(vo.view(np.uint64), g.voxels().view(np.uint64))


@pytest.mark.parametrize("mode", ["scan", "lists", "all_dense"])
@pytest.mark.parametrize("name", sc.PARITY_CASES)
def test_non_incremental_sweeps(name, mode):
    cfg = sc.config(name)
    o, g = pu.make_pair(cfg, PARAMS, synth.noise_table())
    S = 1 << cfg["p_n"]
    V = 1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])
    if mode == "all_dense":
        st = random_state(cfg, 7, run=8, kinds=(0.0, 0.0, 1.0))
    else:
        g.force_sweep_lists(1 if mode == "lists" else 0)
        st = random_state(cfg, 5, run=8 if mode == "lists" else 1)
    (sx, sy, sz), ring = stamps_for(o)
    assert (sx == 2).any() and (sy == 3).any() and (sz == 2).any() and (sx == 0).any() and (sz == 0).any()
    for m in (o, g):
        m.load_state(st)
        m.set_stamps(sx, sy, sz)
        m.set_ring_state(ring)
    hints, seen = [], set()
    for t, depth, cloud, pos, q, mv, remove in sc.drive(name, PARAMS, 4, seed=23):
        for m in (o, g):
            m.set_params(PARAMS)     # every frame ends in a non-incremental sweep
        o.update(depth, cloud, pos, q, mv, remove)
        g.update(depth, cloud, pos, q, mv, remove, sync=True)
        rep = pu.compare_maps(o, g, S, check_results=True, tag="%s %s frame %d: " % (name, mode, t))
        assert not rep, "\n".join(rep)
        hints.append(g.hinted_groups())
        seen |= set(np.sign(o.voxels()["occ"]).tolist())
    assert seen == {-1, 0, 1}, seen      # occupied, free and unknown results all occurred
    if mode == "all_dense":
        # hints are for whole groups of 512 voxels only: a map of fewer has none, a larger one some after the first sweep
        assert (hints[0] == 0) if V < 512 else (0 < hints[0] <= V // 512), (hints, V)
    g.close()


def _block_cap(idx):
    """a cap that ends in the middle of one workgroup's share of the list (k_emit_write: 2048 voxels a workgroup)"""
    blk = np.asarray(idx) // 2048
    b, cnt = np.unique(blk, return_counts=True)
    k = int(np.argmax(cnt))
    return int((blk < b[k]).sum()) + max(1, int(cnt[k]) // 2)


@pytest.mark.parametrize("name", sc.PARITY_CASES)
def test_emitted_lists(name):
    cfg, o, g, reps, _, _, cam = _driven(name)
    assert not reps
    vo = o.voxels()
    ring = g.ring_state()
    assert ring == o.ring_state()
    v0 = int(np.flatnonzero(vo["occ"] != 0)[0])
    assert np.array_equal(sc.emit_positions(cfg, ring, [v0])[0].view(np.uint32), o.voxel_to_pos(v0).view(np.uint32))
    for free in (False, True):
        want = np.flatnonzero(vo["occ"] == 0) if free else np.flatnonzero(vo["occ"] > 0)
        n = len(want)
        assert n >= (1 if name == "A" else 100), (free, n)
        for zero_center in (False, True):
            pts, got_n = g.occupied(free=free, zero_center=zero_center, mark_fov=True)
            assert got_n == n and len(pts) == n, (free, got_n, n)
            for k in ("track", "label"):
                assert np.array_equal(pts[k], vo[k][want]), (free, k)
            assert np.array_equal(pts["occ"] & 0x3f, vo["occ"][want]), free
            sub = cam if zero_center else (0.0, 0.0, 0.0)
            pos = sc.emit_positions(cfg, ring, want, sub)
            got = np.stack([pts["x"], pts["y"], pts["z"]], 1)
            assert np.array_equal(got.view(np.uint32), pos.view(np.uint32)), (free, zero_center)
            corner = sc.emit_positions(cfg, ring, want)
            oof = np.array([not o.point_in_frustum(*c) for c in corner])
            assert np.array_equal((pts["occ"] & 0x40) != 0, oof), (free, zero_center)
        full, _ = g.occupied(free=free)
        for cap in sorted({1, max(1, n - 1), _block_cap(want)}):
            part, got_n = g.occupied(free=free, cap=cap)
            assert got_n == n and len(part) == min(cap, n), (free, cap, got_n)
            assert np.array_equal(part.view(np.uint8), full[:cap].view(np.uint8)), (free, cap)


# ---- queries and the distance field
def _driven_map(name):
    cfg, o, g, reps, eqs, n_occ, _ = _driven(name)
    assert not reps, "\n".join(reps)
    ring = g.ring_state()
    assert sum(e != 0 for e in ring["eq_steps"]) >= (2 if name in ("A", "C") else 3), ring
    return cfg, g, qr.Geometry(cfg, ring), g.voxels()


def _edt(obst):
    try:
        import scipy.ndimage as nd
    except ImportError:
        return er.edt_d2(obst)
    if not obst.any():
        return np.full(obst.shape, er.INVALID, np.uint32)
    idx = nd.distance_transform_edt(~obst, return_distances=False, return_indices=True)
    return sum((idx[a] - np.indices(obst.shape)[a]).astype(np.int64) ** 2 for a in range(3)).astype(np.uint32)


def _reference_d2(obst):
    """brute force where it is cheap (exact, and independent of the min-plus transform), else the transform"""
    n = int(obst.sum())
    if n * obst.size <= 4e7:
        return er.brute_d2(obst)
    return er.edt_d2(obst) if obst.size <= 300000 else _edt(obst)


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_queries_on_driven_maps(name):
    cfg, g, geo, vox = _driven_map(name)
    rng = np.random.default_rng(31)
    size = np.float32(cfg["voxel_size"])
    lo, hi = _span(geo, 2)
    p = rng.uniform(lo, hi, (50000, 3)).astype(np.float32)
    p[:100] = geo.center + geo.pmin
    p[100:200] = geo.center - geo.pmin
    res, idx = g.query_points(p, with_index=True)
    ref, ref_idx = qr.query_points(geo, vox, p)
    assert np.array_equal(idx, ref_idx) and np.array_equal(res.view(np.uint64), ref.view(np.uint64))
    assert (res["occ"] >= (0 if name == "A" else 1)).any() and (res["occ"] == 0).any() and (res["occ"] == -1).any()
    a = rng.uniform(lo, hi, (10000, 3)).astype(np.float32)
    b = rng.uniform(lo, hi, (10000, 3)).astype(np.float32)
    b[:5000] = a[:5000] + rng.normal(0, 3 * size, (5000, 3)).astype(np.float32)
    ha, hb = _hand_segments(geo)
    a, b = np.concatenate([a, ha]), np.concatenate([b, hb])
    for ub in (False, True):
        got = g.query_segments(a, b, unknown_blocks=ub)
        _, ok = _check_segments(geo, vox, got, a, b, ub)
        assert ok.mean() > 0.5 and (got["voxel"][ok] != qr.INVALID).any()
    blo = rng.uniform(lo, hi, (3000, 3)).astype(np.float32)
    bhi = (blo + rng.random((3000, 3)).astype(np.float32) * 6 * size).astype(np.float32)
    blo[0], bhi[0] = geo.center + geo.pmin, geo.center - geo.pmin - np.float32(1e-3) * size
    got = g.query_boxes(blo, bhi)
    ref = qr.query_boxes(geo, vox, blo, bhi)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    assert got["n_occupied"][0] + got["n_free"][0] + got["n_unknown"][0] == len(vox)
    # the distance field under every flag combination, and the distance query
    snap = er.snapshot_grid(geo, vox)
    q = _query_points(geo, rng, 40000)
    for flags in FLAGS:
        g.esdf_update(**_flag_kw(flags))
        d2, site, origin = g.esdf()
        obst = er.obstacle_grid(geo, vox, cfg["max_movable_track"], flags)
        assert not obst.all()
        if not obst.any():   # (only case A's 64 cells may hold no obstacle under a flag)
            assert name == "A" and (d2 == er.INVALID).all() and (site == er.INVALID).all()
            continue
        ref = _edt(obst) if obst.size > 300000 else er.edt_d2(obst)
        bad = np.argwhere(d2 != ref)
        assert not len(bad), (flags, len(bad), bad[:5])
        assert er.check_sites(obst, d2, site, geo.n_bits) is None
        assert np.array_equal(origin, (geo.center + geo.pmin).astype(np.float32))
        _check_query(geo, size, d2, site, snap, obst, q, g.query_distance(q))


def _crafted(name, pattern):
    """oracle and library loaded with a crafted pattern on a ring shifted by crafted_steps, one frame that sees nothing
    (the non-incremental sweep writes every result) -> cfg, g, geo, voxels, (occupied, unknown, tracks)"""
    cfg = sc.config(name)
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    occ_cells, unk_cells, tracks = sc.patterns(cfg, ring)[pattern]
    labels = None if tracks is None else np.where(tracks <= cfg["max_movable_track"], synth.LABEL_CAR, synth.LABEL_BUILDING).astype(np.uint8)
    st = sc.crafted_state(cfg, ring, occ_cells, unk_cells, tracks, labels)
    o, g = pu.make_pair(cfg, PARAMS, synth.noise_table())
    for m in (o, g):
        m.load_state(st)
        m.set_ring_state(ring)
    depth = np.full((cfg["height"], cfg["width"]), np.nan, np.float32)
    cloud = np.zeros(cfg["height"] * cfg["width"], synth.LABELED_POINT)
    cam = np.array(ring["last_pos"], np.float32)
    q = synth.yaw_quat(0.0).astype(np.float32)
    o.update(depth, cloud, cam, q, None)
    g.update(depth, cloud, cam, q, None, sync=True)
    rep = pu.compare_maps(o, g, 1 << cfg["p_n"], check_results=True)
    assert not rep, "\n".join(rep)
    got_ring = g.ring_state()
    assert got_ring["eq_steps"] == ring["eq_steps"] and got_ring["map_center"] == ring["map_center"], (got_ring, ring)
    geo = qr.Geometry(cfg, got_ring)
    vox = g.voxels()
    # the pattern is what the map holds: occupied where placed, unknown where unstamped, free elsewhere
    grid = vox["occ"][geo.voxel_grid()]
    want = np.zeros(grid.shape, np.int8)
    if len(unk_cells):
        want[unk_cells[:, 2], unk_cells[:, 1], unk_cells[:, 0]] = -1
    if len(occ_cells):
        want[occ_cells[:, 2], occ_cells[:, 1], occ_cells[:, 0]] = 1
    assert np.array_equal(grid, want), pattern
    return cfg, g, geo, vox, (occ_cells, unk_cells, tracks)


PATTERN_FLAGS = {"corner": [0], "opposite_corners": [0], "full_line": [0], "alternate": [0], "wrap": [0, er.UNKNOWN_IS_OBSTACLE],
                 "unknown_only": [0, er.UNKNOWN_IS_OBSTACLE], "tracks": [0, er.STATIC_ONLY, er.STATIC_ONLY | er.UNKNOWN_IS_OBSTACLE]}


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_crafted_patterns(name):
    seen_far, seen_wrap = False, False
    for pattern, flag_list in PATTERN_FLAGS.items():
        cfg, g, geo, vox, (occ_cells, unk_cells, tracks) = _crafted(name, pattern)
        assert all(e != 0 for e in geo.eq) and any(abs(int(e)) == int(n) - 1 for e, n in zip(geo.eq, geo.N))
        size = np.float32(cfg["voxel_size"])
        snap = er.snapshot_grid(geo, vox)
        rng = np.random.default_rng(len(pattern))
        for flags in flag_list:
            g.esdf_update(**_flag_kw(flags))
            d2, site, _ = g.esdf()
            obst = er.obstacle_grid(geo, vox, cfg["max_movable_track"], flags)
            if pattern == "unknown_only" and flags == 0:
                assert not obst.any() and (d2 == er.INVALID).all() and (site == er.INVALID).all()
                continue
            assert obst.any()
            if pattern == "tracks" and flags & er.STATIC_ONLY:
                assert int(obst.sum()) == int((tracks > cfg["max_movable_track"]).sum())
            ref = _reference_d2(obst)
            bad = np.argwhere(d2 != ref)
            assert not len(bad), (pattern, flags, len(bad), bad[:5], d2[tuple(bad[0])], ref[tuple(bad[0])])
            assert er.check_sites(obst, d2, site, geo.n_bits) is None, (pattern, flags)
            if int(d2[d2 != er.INVALID].max()) >= 511 ** 2:
                seen_far = True
            if pattern == "wrap":
                seen_wrap = True
                if obst.size <= 300000:   # obstacles on both sides of every axis' wrap point: a torus field would differ
                    assert not np.array_equal(er.edt_d2(obst, periodic=(0, 1, 2)), d2)
            # distance queries: every cell centre (a sample of them on the largest maps), random points
            gz, gy, gx = np.indices(obst.shape)
            cells = np.stack([gx, gy, gz], -1).reshape(-1, 3)
            if len(cells) > 300000:
                cells = cells[rng.choice(len(cells), 300000, replace=False)]
            centres = (geo.center + geo.pmin) + (cells.astype(np.float32) + np.float32(0.5)) * size
            p = np.concatenate([centres, _query_points(geo, rng, 20000)])
            _check_query(geo, size, d2, site, snap, obst, p, g.query_distance(p))
        # segments along the longest axis through the wrap point, boxes spanning the whole axis
        ax = int(np.argmax(geo.N))
        wrap = int((geo.N[ax] - geo.eq[ax]) % geo.N[ax])
        c0 = geo.center + geo.pmin
        a = np.tile(c0 + (geo.N // 2).astype(np.float32) * size + np.float32(0.37) * size, (64, 1)).astype(np.float32)
        b = a.copy()
        a[:, ax] = c0[ax] + (np.float32(wrap) - np.float32(3.3) - np.arange(64, dtype=np.float32) % 7) * size
        b[:, ax] = c0[ax] + (np.float32(wrap) + np.float32(3.6) + np.arange(64, dtype=np.float32) % 5) * size
        a[32:, ax], b[32:, ax] = c0[ax] + np.float32(0.2) * size, c0[ax] + (np.float32(geo.N[ax]) - np.float32(0.3)) * size
        a[32:, (ax + 1) % 3] = b[32:, (ax + 1) % 3] = c0[(ax + 1) % 3] + (np.arange(32, dtype=np.float32) % geo.N[(ax + 1) % 3] + np.float32(0.5)) * size
        for ub in (False, True):
            _check_segments(geo, vox, g.query_segments(a, b, unknown_blocks=ub), a, b, ub)
        blo = np.tile(c0, (16, 1)).astype(np.float32)
        bhi = blo + (rng.random((16, 3)).astype(np.float32) * geo.N.astype(np.float32)) * size
        bhi[:, ax] = c0[ax] + np.float32(geo.N[ax]) * size * np.float32(0.9999)
        blo[8:] -= size * np.float32(2.5)
        got = g.query_boxes(blo, bhi)
        ref = qr.query_boxes(geo, vox, blo, bhi)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (pattern, k)
        g.close()
    assert seen_wrap
    if name == "E":
        assert seen_far


# ---- queries of more than one chunk (2^20 items)
CHUNK = 1 << 20


def _borders(n):
    rows = [r for c in range(CHUNK, n, CHUNK) for r in range(c - 3, c + 3)] + list(range(n - 3, n))
    return np.array(sorted(set(rows)))


def test_queries_longer_than_one_chunk():
    cfg, g, geo, vox = _driven_map("B")
    g.esdf_update()
    d2, site, _ = g.esdf()
    obst = er.obstacle_grid(geo, vox, cfg["max_movable_track"], 0)
    snap = er.snapshot_grid(geo, vox)
    size = np.float32(cfg["voxel_size"])
    rng = np.random.default_rng(41)
    lo, hi = _span(geo, 2)
    n_host, n_dev = CHUNK + 5, 2 * CHUNK + 3

    def inputs(n):
        p = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
        e = (p + rng.normal(0, 4 * size, (n, 3)).astype(np.float32)).astype(np.float32)
        bx = np.concatenate([p, (p + rng.random((n, 3)).astype(np.float32) * 4 * size).astype(np.float32)], 1)
        return p, np.ascontiguousarray(np.concatenate([p, e], 1)), np.ascontiguousarray(bx)

    def small(fn, x, step=200003):
        return np.concatenate([fn(x[s:s + step]) for s in range(0, len(x), step)])

    def check_rows(rows, p, ab, bx, pts, idx, seg, box, dist):
        ref, ref_idx = qr.query_points(geo, vox, p[rows])
        assert np.array_equal(pts[rows].view(np.uint64), ref.view(np.uint64)) and np.array_equal(idx[rows], ref_idx)
        _check_segments(geo, vox, seg[rows], ab[rows, :3], ab[rows, 3:], False)
        ref = qr.query_boxes(geo, vox, bx[rows, :3], bx[rows, 3:])
        for k in ref:
            assert np.array_equal(box[k][rows], ref[k]), k
        _check_query(geo, size, d2, site, snap, obst, p[rows], dist[rows])

    # host mode: the staging area is sized by the segments (the largest rows) and reused by the calls after it
    p, ab, bx = inputs(n_host)
    seg = g.query_segments(ab[:, :3], ab[:, 3:])
    pts, idx = g.query_points(p, with_index=True)
    box = g.query_boxes(bx[:, :3], bx[:, 3:])
    dist = g.query_distance(p)
    assert np.array_equal(seg.view(np.uint8), small(lambda x: g.query_segments(x[:, :3], x[:, 3:]), ab).view(np.uint8))
    assert np.array_equal(pts.view(np.uint8), small(g.query_points, p).view(np.uint8))
    assert np.array_equal(idx, small(lambda x: g.query_points(x, with_index=True)[1], p))
    assert np.array_equal(box.view(np.uint8), small(lambda x: g.query_boxes(x[:, :3], x[:, 3:]), bx).view(np.uint8))
    assert np.array_equal(dist.view(np.uint8), small(g.query_distance, p).view(np.uint8))
    rows = np.concatenate([_borders(n_host), rng.choice(n_host, 3000, replace=False)])
    check_rows(rows, p, ab, bx, pts, idx, seg, box, dist)
    assert (pts["occ"][rows] >= 1).any() and (dist["d2"][rows] != er.INVALID).any()

    # device mode: every chunk's offsets into the inputs and both outputs
    p, ab, bx = inputs(n_dev)
    ins = [g.device_put(x) for x in (p, ab, bx)]
    sizes = (n_dev * 8, n_dev * 4, n_dev * 16, n_dev * 20, n_dev * 36)
    outs = [g.device_alloc(s) for s in sizes]
    g.query_points(ins[0], on_device=True, n=n_dev, out=outs[0], voxel_out=outs[1])
    g.query_segments(ins[1], on_device=True, n=n_dev, out=outs[2])
    g.query_boxes(ins[2], on_device=True, n=n_dev, out=outs[3])
    g.query_distance(ins[0], on_device=True, n=n_dev, out=outs[4])
    g.synchronize()
    dts = (binding.VOXEL_RESULT, np.uint32, binding.SEGMENT_HIT, binding.BOX_RESULT, binding.DISTANCE_RESULT)
    pts, idx, seg, box, dist = [g.device_download(o, s).view(dt) for o, s, dt in zip(outs, sizes, dts)]
    assert np.array_equal(pts.view(np.uint8), small(g.query_points, p, 400009).view(np.uint8))
    assert np.array_equal(idx, small(lambda x: g.query_points(x, with_index=True)[1], p, 400009))
    assert np.array_equal(seg.view(np.uint8), small(lambda x: g.query_segments(x[:, :3], x[:, 3:]), ab, 400009).view(np.uint8))
    assert np.array_equal(box.view(np.uint8), small(lambda x: g.query_boxes(x[:, :3], x[:, 3:]), bx, 400009).view(np.uint8))
    assert np.array_equal(dist.view(np.uint8), small(g.query_distance, p, 400009).view(np.uint8))
    rows = np.concatenate([_borders(n_dev), rng.choice(n_dev, 3000, replace=False)])
    check_rows(rows, p, ab, bx, pts, idx, seg, box, dist)
    for ptr in ins + outs:
        g.device_free(ptr)
