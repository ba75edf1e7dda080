"""The NumPy restatement of the forecast (tests/forecast_ref.py) against brute force, on the CPU: the bit planes per track
and horizon as translated cell sets, `first` against a sort of all landings, the swept lines' connectivity and symmetry,
and the space-time walk without motions against query_ref.query_segments cell for cell."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import forecast_ref as fc
from tests import query_ref as qr
from tests import shape_cases as sc

HORIZONS = np.array([0.25, 0.5, 1.0, 2.0, 4.0], np.float32)


def random_map(name, seed, n_tracks=5):
    """-> (cfg, geo, voxels): a result array drawn free / unknown / occupied 0.5 / 0.2 / 0.3 (a tenth of the occupied
    guessed, occ 2) on a shifted ring, the occupied cells spread over n_tracks movable tracks and a static one"""
    cfg = sc.config(name)
    geo = qr.Geometry(cfg, sc.crafted_ring(cfg, sc.crafted_steps(cfg)))
    rng = np.random.default_rng(seed)
    V = int(geo.N.prod())
    vox = np.zeros(V, binding.VOXEL_RESULT)
    vox["occ"] = rng.choice(np.array([0, -1, 1, 2], np.int8), V, p=[0.5, 0.2, 0.27, 0.03])
    vox["track"] = np.where(vox["occ"] >= 1, rng.choice(np.concatenate([np.arange(1, n_tracks + 1), [60000]]), V), 0)
    return cfg, geo, vox


def test_bit_planes_are_translated_cell_sets():
    cfg, geo, vox = random_map("B", 3)
    mo = fc.motions([2, 4, 5, 9], [[0.3, 0, 0], [-0.2, 0.9, 0.1], [0, -2.5, 1.7], [1, 1, 1]])   # (track 9 has no cell; 1 and 3 stay)
    ref = fc.Field(geo, vox, cfg["voxel_size"], mo, HORIZONS)
    occ, track = fc.grids(geo, vox)
    cls = (ref.mask >> 16) & 3
    assert np.array_equal(cls == 0, occ == -1) and np.array_equal(cls == 1, occ == 0)
    assert np.array_equal(cls == 3, (occ >= 1) & np.isin(track, [2, 4, 5])) and np.array_equal(cls == 2, (occ >= 1) & ~np.isin(track, [2, 4, 5]))
    assert (occ == 2).any() and (ref.mask >> 18 == 0).all()
    NZ, NY, NX = occ.shape
    planes = np.zeros((len(HORIZONS),) + occ.shape, bool)
    lost = 0
    for i in range(len(mo)):
        s = fc.shifts(cfg["voxel_size"], mo["v"][i], HORIZONS)
        own = (occ >= 1) & (track == mo["track"][i])
        for k, (dx, dy, dz) in enumerate(s):
            moved = np.zeros_like(own)   # moved[z + dz, y + dy, x + dx] = own[z, y, x], what leaves the block dropped
            axes = ((NZ, dz), (NY, dy), (NX, dx))   # (a shift of an axis' length or more leaves nothing)
            src = own[tuple(slice(min(n, max(0, -d)), max(0, n - max(0, d))) for n, d in axes)]
            moved[tuple(slice(min(n, max(0, d)), max(0, n - max(0, -d))) for n, d in axes)] = src
            planes[k] |= moved
            lost += int(own.sum()) - int(src.sum())
    for k in range(len(HORIZONS)):
        assert np.array_equal((ref.mask >> k) & 1 == 1, planes[k]), k
    assert ref.info["n_marks_out"] == lost > 0 and ref.info["n_marks_in"] + lost == int(cls.ravel().tolist().count(3)) * len(HORIZONS)
    assert ref.info["n_sources"] == (cls == 3).sum() and ref.info["n_marked"] == planes.any(axis=0).sum() and ref.info["n_stamps"] == 20
    cell, m, f = ref.cells()
    assert np.array_equal(cell, np.flatnonzero(planes.any(axis=0).ravel())) and np.array_equal(m, ref.mask.ravel()[cell])


@pytest.mark.parametrize("swept", [False, True])
def test_first_against_a_sort(swept):
    cfg, geo, vox = random_map("C", 5)
    mo = fc.motions([1, 2, 3], [[0.6, 0, 0.3], [-0.6, 0.3, 0], [0.3, 0.3, 2.4]])
    ref = fc.Field(geo, vox, cfg["voxel_size"], mo, HORIZONS, swept)
    occ, track = fc.grids(geo, vox)
    N = geo.N
    rows = []
    for s in fc.stamps(cfg["voxel_size"], mo, HORIZONS, swept):
        cells = np.argwhere((occ >= 1) & (track == s["track"]))[:, ::-1] + s["d"].astype(np.int64)
        cells = cells[((cells >= 0) & (cells < N)).all(axis=1)]
        w = cells[:, 0] + N[0] * (cells[:, 1] + N[1] * cells[:, 2])
        rows.append(np.stack([w, np.full(len(w), (int(s["horizon"]) << 16) | int(s["track"]))], 1))
    rows = np.concatenate(rows)
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    lead = np.concatenate([[True], rows[1:, 0] != rows[:-1, 0]])
    want = np.full(int(N.prod()), fc.NOTHING, np.uint32)
    want[rows[lead, 0]] = rows[lead, 1]
    assert np.array_equal(ref.first.ravel(), want) and len(rows) == ref.info["n_marks_in"]
    assert ((ref.first != fc.NOTHING) == ((ref.mask & 0xFFFF) != 0)).all()
    if swept:   # a swept build marks what the plain one marks, and more
        plain = fc.Field(geo, vox, cfg["voxel_size"], mo, HORIZONS)
        assert (ref.mask & plain.mask == plain.mask).all() and ref.info["n_marked"] > plain.info["n_marked"]


def test_swept_lines_are_connected_and_mirror():
    rng = np.random.default_rng(2)
    for _ in range(200):
        p, q = rng.integers(-40, 41, 3), rng.integers(-40, 41, 3)
        line = fc.swept_line(p, q)
        chain = np.vstack([p[None, :], line])
        assert np.abs(np.diff(chain, axis=0)).max() <= 1 or (p == q).all()   # 26-connected, from p
        assert (line[-1] == q).all() and len(line) == max(1, np.abs(q - p).max())
        assert np.array_equal(fc.swept_line(-p, -q), -line)                   # reversing the velocity mirrors the line
    for v in ([3.1, -0.7, 1.2], [0.0, 2.0, -2.0]):
        a = fc.stamps(0.25, fc.motions([5], [v]), HORIZONS, swept=True)
        b = fc.stamps(0.25, fc.motions([5], [[-x for x in v]]), HORIZONS, swept=True)
        assert np.array_equal(a["d"], -b["d"]) and np.array_equal(a["horizon"], b["horizon"])


def test_the_walk_without_motions_is_the_segment_query():
    for name in ("A", "B", "C"):
        cfg, geo, vox = random_map(name, 8)
        vox["occ"][vox["occ"] >= 1] = np.where(np.random.default_rng(1).random((vox["occ"] >= 1).sum()) < 0.1, 1, 0)   # thin the obstacles out
        ref = fc.Field(geo, vox, cfg["voxel_size"], None, HORIZONS)
        assert ref.info["n_sources"] == 0 and ref.info["n_marked"] == 0 and (ref.first == fc.NOTHING).all()
        rng = np.random.default_rng(7)
        size = np.float32(cfg["voxel_size"])
        lo, hi = geo.center + geo.pmin, geo.center + geo.pmin + geo.N.astype(np.float32) * size
        a = rng.uniform(lo - 2 * size, hi + 2 * size, (400, 3)).astype(np.float32)
        b = rng.uniform(lo - 2 * size, hi + 2 * size, (400, 3)).astype(np.float32)
        ta = rng.uniform(0, 3, 400).astype(np.float32)
        seg = np.concatenate([a, ta[:, None], b, (ta + rng.uniform(0, 2, 400).astype(np.float32))[:, None]], axis=1)
        for ub in (False, True):
            want, walks = qr.query_segments(geo, vox, a, b, unknown_blocks=ub, record=True)
            got, mine = ref.query_segments(seg, unknown_blocks=ub, record=True)
            assert mine == walks
            assert np.array_equal(got["t"], want["t"]) and np.array_equal(got["cells"], want["cells"])
            hit = want["voxel"] != qr.INVALID
            assert np.array_equal(got["cell"] != fc.NOTHING, hit)
            c = got["cell"][hit].astype(np.int64)
            cells = np.stack([c % geo.N[0], (c // geo.N[0]) % geo.N[1], c // (geo.N[0] * geo.N[1])], 1)
            assert np.array_equal(geo.voxel(cells), want["voxel"][hit])
            assert np.array_equal(got["state"][hit], np.where(want["occ"][hit] >= 1, 1, -1)) and (got["horizon"] == 0xFF).all()
