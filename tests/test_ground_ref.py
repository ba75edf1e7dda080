"""tests/ground_ref.py, the NumPy restatement the GPU tests hold the ground layer to, against the contract of
include/sdm.h written out as plain loops: one column at a time, one neighbour at a time, and a brute-force search for the
nearest lethal column.  Random blocks of at most 16 cells per axis; no GPU."""
import itertools
import math

import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import esdf_ref as er
from tests import ground_ref as gr

MAX_MOVABLE = 20
ORIENTATIONS = [(a, s) for a in (0, 1, 2) for s in (1, -1)]


def random_snap(rng, shape):
    """[z, y, x] result words: occ in {-1, 0, 1, 2}, a handful of labels, movable and static tracks"""
    occ = rng.choice(np.array([-1, 0, 0, 1, 1, 2], np.int64), size=shape)
    label = rng.choice(np.array([0, 3, 7, 40, 255]), size=shape)
    track = rng.choice(np.array([0, 1, 5, MAX_MOVABLE, MAX_MOVABLE + 1, 900, 65535]), size=shape)
    known = occ >= 1
    w = np.where(known, track | (label << 16), 0) | ((occ & 0xFF) << 24)
    return w.astype(np.uint32)


def loop_build(snap, opt):
    """the contract, cell by cell"""
    NZ, NY, NX = snap.shape
    N = (NX, NY, NZ)
    axis, sign = opt["up"]
    au, av = gr.grid_axes(axis)
    NA, NU, NV = N[axis], N[au], N[av]
    fl = opt["flags"]

    def word(i, j, h):
        idx = [0, 0, 0]
        idx[axis], idx[au], idx[av] = (h if sign > 0 else NA - 1 - h), i, j
        return int(snap[idx[2], idx[1], idx[0]])

    def parts(w):
        occ = (w >> 24) & 0xFF
        return w & 0xFFFF, (w >> 16) & 0xFF, occ - 256 if occ >= 128 else occ

    def movable(w):
        return 1 <= parts(w)[0] <= MAX_MOVABLE

    def solid(w):
        return parts(w)[2] >= 1 and not ((fl & gr.IGNORE_MOVABLE) and movable(w))

    def passable(i, j, h):
        if h >= NA:
            return True
        w = word(i, j, h)
        occ = parts(w)[2]
        return occ == 0 or (occ >= 1 and not solid(w)) or (bool(fl & gr.UNKNOWN_PASSABLE) and occ == -1)

    def support(i, j, h):
        w = word(i, j, h)
        return (solid(w) and not movable(w) and parts(w)[1] in opt["labels"]
                and all(passable(i, j, k) for k in range(h + 1, h + opt["clearance"] + 1)))

    cells = np.zeros((NV, NU), binding.GROUND_CELL)
    for j in range(NV):
        for i in range(NU):
            band = range(opt["h_lo"], opt["h_hi"] + 1)
            sup = [h for h in band if support(i, j, h)]
            sol = [h for h in band if solid(word(i, j, h))]
            c = cells[j, i]
            c["level"], c["top"] = (max(sup) if sup else gr.NO_LEVEL), (max(sol) if sol else gr.NO_LEVEL)
            if sup:
                c["label"] = parts(word(i, j, max(sup)))[1]
                room = 0
                while max(sup) + room + 1 < NA and passable(i, j, max(sup) + room + 1):
                    room += 1
                c["headroom"] = min(room, 255)
            c["n_unknown"] = min(sum(parts(word(i, j, h))[2] == -1 for h in band), 255)
            c["cls"] = 1 if sup else (2 if sol else 0)
    for j in range(NV):
        for i in range(NU):
            c = cells[j, i]
            step = False
            for qi, qj in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                if 0 <= qi < NU and 0 <= qj < NV and c["level"] != gr.NO_LEVEL and cells[qj, qi]["level"] != gr.NO_LEVEL:
                    step = step or int(c["level"]) > int(cells[qj, qi]["level"]) + opt["max_step"]
            k = int(c["cls"]) & 3
            lethal = k == 2 or step or (k == 0 and bool(fl & gr.NONE_IS_LETHAL))
            c["cls"] = k | (4 if step else 0) | (8 if lethal else 0)
    sites = [(i, j) for j in range(NV) for i in range(NU) if cells[j, i]["cls"] & 8]
    d2 = np.full((NV, NU), gr.INVALID, np.uint32)
    for j in range(NV):
        for i in range(NU):
            if sites:
                d2[j, i] = min((i - si) ** 2 + (j - sj) ** 2 for si, sj in sites)
    return cells, d2


@pytest.mark.parametrize("up", ORIENTATIONS)
def test_build_against_the_loops(up):
    rng = np.random.default_rng(100 + 10 * up[0] + up[1])
    shapes = [(16, 8, 4), (4, 16, 8), (8, 4, 16), (5, 6, 7)]   # [z, y, x]; the reference needs no powers of two
    for shape, flags in zip(itertools.cycle(shapes), range(8)):
        snap = random_snap(rng, shape)
        NA = shape[2 - up[0]]
        for clearance in (0, 1, 40):               # 40: larger than any block
            for max_step in (0, 65535):
                lo = int(rng.integers(0, NA))
                hi = int(rng.integers(lo, NA))
                labels = [[3, 7], [0, 3, 7, 40, 255], []][int(rng.integers(0, 3))]
                opt = gr.options(up, lo, hi, clearance, max_step, labels, flags)
                cells, d2, info = gr.build(snap, MAX_MOVABLE, opt)
                want_cells, want_d2 = loop_build(snap, opt)
                for name in binding.GROUND_CELL.names:
                    assert np.array_equal(cells[name], want_cells[name]), (name, shape, opt)
                assert np.array_equal(d2, want_d2), (shape, opt)
                k = want_cells["cls"]
                assert (info["n_ground"], info["n_obstacle"], info["n_none"]) == tuple(int(((k & 3) == c).sum()) for c in (1, 2, 0))
                assert (info["n_step"], info["n_lethal"]) == (int(((k & 4) != 0).sum()), int(((k & 8) != 0).sum()))
                lv = want_cells["level"][want_cells["level"] != gr.NO_LEVEL]
                assert (info["level_min"], info["level_max"]) == ((int(lv.min()), int(lv.max())) if len(lv) else (gr.NO_LEVEL,) * 2)
                au, av = gr.grid_axes(up[0])
                assert (info["n_u"], info["n_v"], info["axis_u"], info["axis_v"]) == (shape[2 - au], shape[2 - av], au, av)


def test_a_step_marks_the_higher_side_only():
    snap = np.zeros((1, 4, 4), np.uint32)          # up y (sign +): a row of columns along x, levels 0, 0, 2, 3
    solid = np.uint32(900 | (7 << 16) | (1 << 24))
    for x, h in enumerate((0, 0, 2, 3)):
        snap[0, h, x] = solid
    for max_step, want in ((1, [0, 0, 1, 0]), (2, [0, 0, 0, 0]), (0, [0, 0, 1, 1])):
        cells, d2, info = gr.build(snap, MAX_MOVABLE, gr.options((1, 1), 0, 3, 0, max_step, [7]))
        assert list((cells["cls"][0] >> 2) & 1) == want and list((cells["cls"][0] >> 3) & 1) == want
        assert list(d2[0]) == ([(2 - x) ** 2 for x in range(4)] if max_step == 1 else [gr.INVALID] * 4 if max_step == 2 else [4, 1, 0, 0])


def _geo(n_bits, size, center=(0.3, -1.2, 2.0)):
    return er.geometry(n_bits, size, center=center, eq=(1, 2, 3))


def test_footprint_rule_on_rotated_rectangles():
    geo, size = _geo((4, 3, 4), 0.25), 0.25
    rng = np.random.default_rng(5)
    snap = random_snap(rng, (16, 8, 16))
    for up in ORIENTATIONS:
        opt = gr.options(up, 0, int(geo.N[up[0]]) - 1, 1, 1, [3, 7])
        cells, d2, _ = gr.build(snap, MAX_MOVABLE, opt)
        au, av = gr.grid_axes(up[0])
        o = gr.origin_of(geo)
        fps = np.zeros(8, binding.FOOTPRINT)
        for k in range(8):
            th = [0.0, math.pi / 2, math.pi, 0.4, 1.1, 2.5, -0.7, 4.0][k]
            fps[k] = (o[au] + rng.uniform(0, geo.N[au] * size), o[av] + rng.uniform(0, geo.N[av] * size), math.cos(th), math.sin(th),
                      rng.uniform(0.2, 1.5), rng.uniform(0.1, 0.8))
        fps[1]["dir_u"], fps[1]["dir_v"] = 0.0, 1.0      # exactly along v
        fps[7] = (o[au] + 1.0 * size, o[av] + 1.0 * size, 1.0, 0.0, 0.1 * size, 0.1 * size)   # on a corner of four columns: covers no centre
        got = gr.query_footprints(geo, size, opt, cells, d2, fps)
        for k, fp in enumerate(fps):
            n = dict(n_cols=0, n_lethal=0, n_none=0, n_ground=0)
            levels, dists, lethal = [], [], []
            for j in range(int(geo.N[av])):
                for i in range(int(geo.N[au])):
                    f32 = np.float32
                    pu = f32(o[au] + f32(f32(f32(i) + f32(0.5)) * f32(size)))
                    pv = f32(o[av] + f32(f32(f32(j) + f32(0.5)) * f32(size)))
                    du, dv = f32(pu - fp["center_u"]), f32(pv - fp["center_v"])
                    along = f32(f32(du * fp["dir_u"]) + f32(dv * fp["dir_v"]))
                    across = f32(f32(dv * fp["dir_u"]) - f32(du * fp["dir_v"]))
                    if not (abs(along) <= fp["half_len"] and abs(across) <= fp["half_wid"]):
                        continue
                    c = cells[j, i]
                    n["n_cols"] += 1
                    n["n_lethal"] += int(c["cls"] >> 3) & 1
                    n["n_none"] += int((c["cls"] & 3) == 0)
                    n["n_ground"] += int((c["cls"] & 3) == 1)
                    dists.append(int(d2[j, i]))
                    if (c["cls"] & 3) == 1:
                        levels.append(int(c["level"]))
                    if c["cls"] & 8:
                        lethal.append(i + j * int(geo.N[au]))
            want = (n["n_cols"], n["n_lethal"], n["n_none"], n["n_ground"], min(levels, default=gr.NO_LEVEL), max(levels, default=gr.NO_LEVEL),
                    min(dists, default=gr.INVALID), min(lethal, default=gr.INVALID), 0)
            assert tuple(int(v) for v in got[k]) == want, (up, k)
        assert got["n_cols"][7] == 0 and got["n_cols"][:7].min() > 0
        # axis-aligned: a rectangle of whole columns, counted by hand
        fp = np.zeros(1, binding.FOOTPRINT)
        fp[0] = (o[au] + 4 * size, o[av] + 3 * size, 1.0, 0.0, 2 * size, 1 * size)
        assert gr.query_footprints(geo, size, opt, cells, d2, fp)["n_cols"][0] == 4 * 2


def test_footprints_that_answer_nothing():
    geo, size = _geo((3, 3, 3), 0.5), 0.5
    snap = random_snap(np.random.default_rng(6), (8, 8, 8))
    opt = gr.options((2, 1), 0, 7, 0, 0, [3])
    cells, d2, _ = gr.build(snap, MAX_MOVABLE, opt)
    fps = np.zeros(4, binding.FOOTPRINT)
    fps[:] = (0.0, 0.0, 1.0, 0.0, 1.0, 0.5)
    fps[1]["half_len"], fps[1]["half_wid"] = 41.5 * size, 23.0 * size     # too large: half_len + half_wid > 64 * size
    fps[2]["dir_v"] = np.nan
    fps[3]["center_u"] = np.inf
    got = gr.query_footprints(geo, size, opt, cells, d2, fps)
    assert got["n_cols"][0] > 0
    for k in (1, 2, 3):
        assert tuple(int(v) for v in got[k]) == (0, 0, 0, 0, gr.NO_LEVEL, gr.NO_LEVEL, gr.INVALID, gr.INVALID, 0)
    fps[1]["half_len"] = 41.0 * size            # 64 voxels, just allowed: covers the whole small grid
    assert gr.query_footprints(geo, size, opt, cells, d2, fps)["n_cols"][1] == 64


def test_point_query_against_single_points():
    geo, size = _geo((3, 4, 2), 0.5), 0.5
    rng = np.random.default_rng(7)
    snap = random_snap(rng, (4, 16, 8))
    for up in ORIENTATIONS:
        opt = gr.options(up, 0, int(geo.N[up[0]]) - 1, 0, 0, [3, 7, 40])
        cells, d2, _ = gr.build(snap, MAX_MOVABLE, opt)
        o = gr.origin_of(geo).astype(np.float64)
        pts = o + rng.uniform(-1.0, 1.0, (200, 3)) * size + rng.uniform(0, 1, (200, 3)) * geo.N * size
        pts[0], pts[1] = np.nan, np.inf
        pts[2] = o + np.array([-0.5, 0.5, 0.5]) * size       # the u in (-1, 0) sliver: outside, unlike query_points' cast
        got = gr.query_ground(geo, size, opt, cells, d2, pts)
        assert list(got["status"][:3]) == [3, 3, 3] and (got["status"] == 0).sum() > 20
        au, av = gr.grid_axes(up[0])
        for r, u in zip(got, geo.u(pts)):
            inside = all(0 <= float(u[a]) < float(geo.N[a]) for a in range(3))
            assert (r["status"] == 0) == inside
            if not inside:
                assert (r["col"], r["d2"], r["surface"], r["above"], r["dist"]) == (gr.INVALID, gr.INVALID, 0, gr.INT32_MIN, -1)
                assert tuple(r["cell"]) == (gr.NO_LEVEL, gr.NO_LEVEL, 0, 0, 0, 0)
                continue
            c = [int(math.floor(float(v))) for v in u]
            assert r["col"] == c[au] + c[av] * int(geo.N[au]) and r["cell"] == cells[c[av], c[au]] and r["d2"] == d2[c[av], c[au]]
            level = int(r["cell"]["level"])
            if level == gr.NO_LEVEL:
                assert r["above"] == gr.INT32_MIN and r["surface"] == 0
            else:
                NA = int(geo.N[up[0]])
                idx = level if up[1] > 0 else NA - 1 - level
                assert r["above"] == (c[up[0]] if up[1] > 0 else NA - 1 - c[up[0]]) - level
                face = idx + 1 if up[1] > 0 else idx
                assert r["surface"] == np.float32(gr.origin_of(geo)[up[0]] + np.float32(np.float32(face) * np.float32(size)))
            want = np.float32(-1) if r["d2"] == gr.INVALID else np.float32(np.sqrt(np.float32(r["d2"])) * np.float32(size))
            assert r["dist"] == want


def test_ground_band():
    cfg = dict(x_n=4, y_n=5, z_n=3, voxel_size=0.5)
    origin = [-4.0, -8.0, -2.0]
    assert binding.ground_band(cfg, origin, (2, 1), -2.0, 1.9) == (0, 7)
    assert binding.ground_band(cfg, origin, (2, 1), -1.0, -0.6) == (2, 2)
    assert binding.ground_band(cfg, origin, (2, 1), -100.0, 100.0) == (0, 7)          # clamped
    assert binding.ground_band(cfg, origin, (1, -1), -8.0, -7.6) == (31, 31)          # -y up: index 0 is the highest cell
    assert binding.ground_band(cfg, origin, (1, -1), 7.0, 7.9) == (0, 1)
    assert binding.ground_band(cfg, origin, (0, 1), 0.0, 0.0) == (8, 8)
    for bad in ((3, 1), (0, 0), (1, 2)):
        with pytest.raises(ValueError):
            binding.ground_band(cfg, origin, bad, 0.0, 1.0)
    with pytest.raises(ValueError):
        binding.ground_band(cfg, origin, (0, 1), 1.0, 0.0)
    assert list(binding.label_mask([0, 31, 32, 255])) == [0x80000001, 1, 0, 0, 0, 0, 0, 1 << 31]
    assert not binding.label_mask(None).any()
