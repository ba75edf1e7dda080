"""CPU checks of tests/shard_cases.py: every case is a sharding sdm_create accepts and has the property it is there for
(planes per slab, voxels per shard against one 64-voxel chunk and one 512-voxel group, shards that own no pixel of the
ck image), and the crafted object of the thin-shard GPU tests is larger than one shard and moves across the ring's z
wrap, more than one slab at a time."""
import numpy as np
import pytest

from semantic_dsp_map_amd import synth
from tests import query_ref as qr
from tests import shape_cases as sc
from tests import shard_cases as shc


@pytest.mark.parametrize("name", list(shc.CASES))
def test_case_has_its_property(name):
    case = shc.CASES[name]
    cfg = shc.config(name)
    G = case["G"]
    assert all(shc.sdm_create_accepts_shard(cfg, r, G) for r in range(G))
    assert not shc.sdm_create_accepts_shard(cfg, G, G) and not shc.sdm_create_accepts_shard(cfg, -1, G)
    assert not shc.sdm_create_accepts_shard(cfg, 0, 3 * G)          # (3 G divides no power of two)
    assert G <= shc.MAX_LIVE_SHARDS
    assert shc.planes(cfg, G) == case["planes"] and shc.planes(cfg, G) * G == 1 << cfg["z_n"]
    n = shc.v_count(cfg, G)
    assert shc.vox_class(n) == case["vox"], (n, case["vox"])
    assert n == shc.planes(cfg, G) << (cfg["x_n"] + cfg["y_n"])
    chunk = shc.ck_chunk(cfg, G)
    hw = cfg["width"] * cfg["height"]
    assert chunk % 64 == 0 and chunk * G >= hw and (chunk - 64) * G < hw
    assert shc.ck_empty_shards(cfg, G) == tuple(case["empty_ck"])
    for k in case["empty_ck"]:
        assert k * chunk >= hw


def test_the_cases_cover_the_properties():
    got = {name: (shc.config(name), c["G"]) for name, c in shc.CASES.items()}
    assert {n for n, (cfg, G) in got.items() if cfg["x_n"] == cfg["y_n"] == cfg["z_n"] == 5} == {"T0/8", "T0/16", "T0/32", "T0cam/32"}
    assert [got["T0/%d" % G][1] for G in (8, 16, 32)] == [8, 16, 32] and shc.planes(*got["T0/32"]) == 1
    assert shc.v_count(*got["A/4"]) == 16 and shc.v_count(*got["B/16"]) == 512 and shc.v_count(*got["B/32"]) == 256
    assert shc.v_count(*got["C/32"]) == 128 and got["C/32"][0]["p_n"] == 4
    d = got["D/8"][0]
    assert shc.planes(d, 8) == 1 and d["y_n"] == 9 and sc.CASES["D"]["tilt"] != 0
    cam = got["T0cam/32"][0]
    assert (cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]) == (48, 40, 30.0, 30.0, 24.0, 20.0)
    assert shc.ck_empty_shards(cam, 32) == (30, 31)
    classes = {c["vox"] for c in shc.CASES.values()}
    assert classes == {"lt64", "lt512", "eq512", "ge512"}
    for name in shc.SHAPE_CASES + shc.SWEEP_CASES:
        assert shc.shape_of(name) in sc.PARITY_CASES


def test_slab_of_matches_the_shard_ranges():
    cfg = shc.config("T0/16")
    V = 1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])
    n = shc.v_count(cfg, 16)
    v = np.arange(V)
    assert np.array_equal(shc.slab_of(cfg, 16, v), v // n)


def _big_destinations(cfg, ring, G):
    """the noise-free target of every member of the crafted object, as (source shard, destination shard) per member"""
    geo = qr.Geometry(cfg, ring)
    cells = shc.big_block(cfg, ring)
    st = shc.big_state(cfg, ring)
    S = 1 << cfg["p_n"]
    src_vox = geo.voxel(cells).astype(np.int64)
    i = src_vox * S + 1
    p = np.stack([st["px"][i], st["py"][i], st["pz"][i]], 1).astype(np.float32)
    T = shc.big_move(cfg, ring)[0]["T"].reshape(4, 4)
    q = (p @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    dst = np.floor(geo.u(q)).astype(np.int64)
    assert ((dst >= 0) & (dst < geo.N)).all()                   # nothing leaves the map
    dst_vox = geo.voxel(dst).astype(np.int64)
    return shc.slab_of(cfg, G, src_vox), shc.slab_of(cfg, G, dst_vox)


def test_the_crafted_object_is_larger_than_a_shard_and_crosses_the_wrap():
    cfg = shc.config("T0/32")
    ring = shc.big_ring(cfg)
    st = shc.big_state(cfg, ring)
    S = 1 << cfg["p_n"]
    V = 1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])
    members = st["owner"] == shc.BIG_TRACK
    assert int(members.sum()) == 17920 == int(np.prod(shc.BIG_BLOCK)) * shc.BIG_SLOTS
    assert (st["track"][members] == shc.BIG_TRACK).all() and shc.BIG_TRACK <= cfg["max_movable_track"]
    assert (st["status"][members] == sc.ST_UPDATED).all() and not (np.flatnonzero(members) % S == 0).any()
    # more than one shard's slots at G = 16 and 32, within the whole map's per-frame capacity of moved copies
    for G in (16, 32):
        assert 17920 > shc.v_count(cfg, G) * S
    assert 17920 <= min(V * S, 1 << 18)
    # the block's ring planes run across the wrap: shard G-1 holds members, and so does shard 0
    rz = np.flatnonzero(members) // S >> (cfg["x_n"] + cfg["y_n"])
    assert set(np.unique(rz)) == {24, 25, 26, 27, 28, 29, 30, 31, 0, 1}
    for G in (16, 32):
        src, dst = _big_destinations(cfg, ring, G)
        dist = (dst - src) % G
        assert (dist >= 2).any() and (dist < G // 2).all()           # more than one slab at a time, one way
        pairs = set(zip(src.tolist(), dst.tolist()))
        assert any(s == G - 1 and d < s for s, d in pairs) and any(d == 0 and s > 0 for s, d in pairs)
    # planes the copies land in: the yaw spreads them over more than one
    src, dst = _big_destinations(cfg, ring, 32)
    assert len(set((dst - src) % 32)) >= 2
    assert (synth.LABEL_CAR == st["label"][members]).all()
