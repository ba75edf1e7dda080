"""CPU checks of tests/shape_cases.py, the ground the GPU shape tests stand on: the cases are grids sdm_create accepts,
crafted cells land where query_ref.Geometry puts them, the distance references agree with each other on the crafted
patterns, the emitted positions' restatement matches the oracle, and query_ref tells the y and z axes apart on every
non-cubic case (so the GPU checks would catch a mix-up of them)."""
import numpy as np
import pytest

from oracle import oracle as orc
from semantic_dsp_map_amd import synth
from tests import esdf_ref as er
from tests import query_ref as qr
from tests import shape_cases as sc
from tests.dense_state import stamp_slabs


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_cases_are_accepted_grids(name):
    cfg = sc.config(name)
    assert sc.sdm_create_accepts(cfg)
    for bad in (dict(x_n=1), dict(z_n=10), dict(p_n=0), dict(p_n=5), dict(x_n=9, y_n=9, z_n=9, p_n=5), dict(voxel_size=0.0)):
        assert not sc.sdm_create_accepts(dict(cfg, **bad))
    for a, b in zip(sc.quat_mat(sc.mat_quat(sc.rot_x(sc.CASES[name]["tilt"]) @ sc.rot_y(0.3))).ravel(),
                    (sc.rot_x(sc.CASES[name]["tilt"]) @ sc.rot_y(0.3)).ravel()):
        assert abs(a - b) < 1e-12
    assert np.allclose(sc.mat_quat(sc.rot_y(0.7)), synth.yaw_quat(0.7))


def test_the_matrix_covers_the_properties():
    n = {k: sc.config(k) for k in sc.ALL_CASES}
    vol = {k: 1 << (c["x_n"] + c["y_n"] + c["z_n"]) for k, c in n.items()}
    assert vol["A"] == 64 and n["A"]["x_n"] < 3                            # below one group, x rows of 4
    assert n["B"]["x_n"] == 2 and vol["B"] > 512                           # x of 4 on many groups
    assert n["C"]["x_n"] == 3 and n["C"]["y_n"] == 2 and n["C"]["p_n"] == 4  # a group is a row; y of 4; 16 slots
    assert n["D"]["y_n"] == 9 and n["D"]["x_n"] < 6
    assert n["E"]["x_n"] == 9 and n["E"]["z_n"] == 9 and vol["E"] == 1 << 21
    ref = synth.CONFIGS["REF_ZED2_BOOST"]
    assert all(n["F"][k] == ref[k] for k in ("x_n", "y_n", "z_n", "p_n", "voxel_size"))


def test_stamp_slabs_keep_the_old_slabs_and_fit_short_axes():
    assert stamp_slabs(32, 32, 32) == (slice(3, 6), 10, slice(20, 22))
    assert stamp_slabs(128, 64, 256) == (slice(3, 6), 10, slice(20, 22))
    for n in (4, 8, 16):
        xs, yi, zs = stamp_slabs(n, n, n)
        for s in (xs, zs):
            assert 0 <= s.start < s.stop < n
        assert 0 <= yi < n


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_crafted_cells_land_where_the_geometry_puts_them(name):
    cfg = sc.config(name)
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    geo = qr.Geometry(cfg, ring)
    assert all(e != 0 for e in geo.eq) and abs(int(geo.eq[0])) == geo.N[0] - 1 and abs(int(geo.eq[1])) == geo.N[1] - 1
    S = 1 << cfg["p_n"]
    for pat, (occ, unk, tracks) in sc.patterns(cfg, ring).items():
        st = sc.crafted_state(cfg, ring, occ, unk, tracks)
        held = np.flatnonzero(st["status"].reshape(-1, S)[:, 1] != 0)
        assert np.array_equal(np.sort(held), np.sort(geo.voxel(occ).astype(np.int64))), pat
        unseen = np.flatnonzero(st["ts"].reshape(-1, S)[:, 0] == 0)
        assert np.array_equal(np.sort(unseen), np.sort(geo.voxel(unk).astype(np.int64))), pat
        # the particle of a cell sits at the cell's centre: the map's own position -> cell mapping finds it
        if len(occ):
            i = held[:5] * S + 1
            p = np.stack([st["px"][i], st["py"][i], st["pz"][i]], 1)
            assert np.array_equal(np.floor(geo.u(p)).astype(np.int64), occ[np.argsort(geo.voxel(occ))][:5])
    # the camera of the crafted frame lies in the cell the ring follows: the frame moves nothing
    steps = np.floor(np.array(ring["last_pos"], np.float32) / np.float32(cfg["voxel_size"])).astype(np.int64)
    assert list(np.where(steps < 0, steps + 1, steps)) == ring["moved_steps"]


def _scipy_d2(obst):
    try:
        import scipy.ndimage as nd
    except ImportError:
        return None
    idx = nd.distance_transform_edt(~obst, return_distances=False, return_indices=True)
    return sum((idx[a] - np.indices(obst.shape)[a]).astype(np.int64) ** 2 for a in range(3)).astype(np.uint32)


@pytest.mark.parametrize("name", ["D", "E"])
def test_distance_references_agree_on_the_crafted_patterns(name):
    """brute_d2, edt_d2 and scipy (where it imports) on D's size in full; on E's (2 M cells, seconds per transform) on
    the x-z plane that holds the pattern, a slab of two y layers, for the patterns whose far cells matter most"""
    cfg = sc.config(name)
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    geo = qr.Geometry(cfg, ring)
    pats = sc.patterns(cfg, ring)
    for pat in ("corner", "opposite_corners", "wrap", "tracks"):
        occ = pats[pat][0]
        obst = np.zeros(tuple(geo.N[::-1]), bool)
        obst[occ[:, 2], occ[:, 1], occ[:, 0]] = True
        if name == "E":
            keep = np.unique(occ[:, 1])[:2]
            obst = obst[:, keep, :]
            if pat != "corner" or not obst.any():
                continue
        b = er.brute_d2(obst)
        assert np.array_equal(b, er.edt_d2(obst)), pat
        s = _scipy_d2(obst)
        if s is not None:
            assert np.array_equal(b, s), pat
    if name == "E":   # the far corner of E: 511^2 + 511^2 in the plane (+ 7^2 across y on the full map)
        assert int(b.max()) == 2 * 511 ** 2


@pytest.mark.parametrize("name", sc.PARITY_CASES)
def test_emit_positions_match_the_oracle(name):
    cfg = sc.config(name)
    o = orc.OracleMap(dict(cfg, bin_order=1), synth.PARAMS["vkitti2"], synth.noise_table())
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    o.set_ring_state(ring)
    V = 1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])
    rng = np.random.default_rng(3)
    vox = np.concatenate([[0, V - 1], rng.integers(0, V, 200)])
    got = sc.emit_positions(cfg, o.ring_state(), vox)
    want = np.stack([o.voxel_to_pos(int(v)) for v in vox])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _swap_yz(geo):
    g = qr.Geometry.__new__(qr.Geometry)
    perm = [0, 2, 1]
    g.n_bits, g.N, g.pmin, g.center, g.eq = geo.n_bits[perm], geo.N[perm], geo.pmin[perm], geo.center[perm], geo.eq[perm]
    g.recip = geo.recip
    return g


@pytest.mark.parametrize("name", ["B", "C", "D", "E", "F"])
def test_query_reference_tells_y_from_z(name):
    """the answers of query_ref with the y and z sizes and offsets swapped differ from the true ones on every non-cubic
    case: a kernel that mixed them up would fail the GPU checks"""
    cfg = sc.config(name)
    ring = sc.crafted_ring(cfg, sc.crafted_steps(cfg))
    geo = qr.Geometry(cfg, ring)
    bad = _swap_yz(geo)
    V = int(np.prod(geo.N))
    rng = np.random.default_rng(9)
    vox = np.zeros(V, orc.VOXEL_RESULT)
    vox["occ"] = rng.choice([-1, 0, 1], V)
    vox["track"] = rng.integers(0, 60000, V)
    size = np.float32(1) / geo.recip
    lo, hi = geo.center + geo.pmin, geo.center - geo.pmin
    p = rng.uniform(lo, hi, (2000, 3)).astype(np.float32)
    r1, i1 = qr.query_points(geo, vox, p)
    r2, i2 = qr.query_points(bad, vox, p)
    assert not np.array_equal(i1, i2)
    a = rng.uniform(lo, hi, (300, 3)).astype(np.float32)
    b = (a + rng.normal(0, 4 * size, (300, 3))).astype(np.float32)
    s1, s2 = qr.query_segments(geo, vox, a, b), qr.query_segments(bad, vox, a, b)
    assert not np.array_equal(s1["voxel"], s2["voxel"])
    blo = rng.uniform(lo, hi, (40, 3)).astype(np.float32)
    bhi = (blo + rng.random((40, 3)).astype(np.float32) * 5 * size).astype(np.float32)
    b1, b2 = qr.query_boxes(geo, vox, blo, bhi), qr.query_boxes(bad, vox, blo, bhi)
    assert any(not np.array_equal(b1[k], b2[k]) for k in b1)
