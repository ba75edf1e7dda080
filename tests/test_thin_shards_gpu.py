"""Thin Z-slab shards (tests/shard_cases.py) against the oracle: slabs of one or two planes, shards of 16 to 512 voxels,
shards that own only ck padding.  G shard maps side by side on one GPU, the test playing the collectives
(tests/test_sharded_gpu.py), the union of the shards bit for bit against the unsharded oracle: free-running frames on
the shape cases and on a small camera, non-incremental sweeps of a random dense state, the emitted clouds in full, and
one frame that moves an object of more members than one shard has slots across the ring's z wrap - with an export
capacity that holds its copies, and with one that drops some of them (reported exactly)."""
import numpy as np
import pytest

from oracle import oracle as orc
from semantic_dsp_map_amd import binding, synth
from tests import parity_utils as pu
from tests import shape_cases as sc
from tests import shard_cases as shc
from tests.dense_state import random_state, stamps_for
from tests.test_shapes_gpu import _block_cap
from tests.test_sharded_gpu import Shard, compare_union, run_frame

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
N_FRAMES = 24
HALO_CAP = 4096    # the library default: the shape cases' objects send more than 1024 copies to one slab in a frame


def _oracle(cfg, G):
    return orc.OracleMap(dict(cfg, bin_order=1, ck_slabs=G), PARAMS, synth.noise_table())


def _shards(cfg, G, halo_cap=HALO_CAP):
    assert G <= shc.MAX_LIVE_SHARDS
    shards = []
    try:
        for r in range(G):
            shards.append(Shard(cfg, PARAMS, synth.noise_table(), r, G, halo_cap))
    except BaseException:
        _close(shards)
        raise
    return shards


def _close(shards):
    for s in shards:
        s.m.close()


def _far(hdr):
    """copies exported to a shard two slabs away or more, either way round the ring"""
    G = len(hdr)
    d = np.abs(np.subtract.outer(np.arange(G), np.arange(G)))
    return int(hdr[np.minimum(d, G - d) >= 2].sum())


def _expected_cloud(cfg, o, want, sub):
    """the emitted POINT records of storage voxels `want`, restated from the oracle's voxels"""
    vo = o.voxels()
    ring = o.ring_state()
    out = np.zeros(len(want), binding.POINT)
    pos = sc.emit_positions(cfg, ring, want, sub)
    out["x"], out["y"], out["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    out["track"], out["label"] = vo["track"][want], vo["label"][want]
    corner = sc.emit_positions(cfg, ring, want)
    oof = np.array([not o.point_in_frustum(*c) for c in corner], bool)
    out["occ"] = vo["occ"][want] | np.where(oof, 0x40, 0).astype(np.int8)
    return out


def _check_emitted(cfg, o, shards, cam):
    """every shard's occupied / free cloud, concatenated in shard order = the whole map's list built from the oracle,
    byte for byte; and per shard, caps of 1, n - 1 and one that ends in the middle of a workgroup's share"""
    vo = o.voxels()
    n_shard = shards[0].m.v_count
    for free in (False, True):
        want = np.flatnonzero(vo["occ"] == 0) if free else np.flatnonzero(vo["occ"] > 0)
        assert len(want) >= 1, free
        for zero_center in (False, True):
            parts = []
            for s in shards:
                pts, n = s.m.occupied(free=free, zero_center=zero_center, mark_fov=True)
                assert n == len(pts)
                parts.append(pts)
            got = np.concatenate(parts)
            exp = _expected_cloud(cfg, o, want, cam if zero_center else (0.0, 0.0, 0.0))
            assert len(got) == len(exp), (free, zero_center, len(got), len(exp))
            assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), (free, zero_center)
        for r, s in enumerate(shards):
            mine = want[(want >= r * n_shard) & (want < (r + 1) * n_shard)] - r * n_shard
            n = len(mine)
            if n == 0:
                continue
            full, _ = s.m.occupied(free=free)
            for cap in sorted({1, max(1, n - 1), _block_cap(mine)}):
                part, got_n = s.m.occupied(free=free, cap=cap)
                assert got_n == n and len(part) == min(cap, n), (r, free, cap, got_n, n)
                assert np.array_equal(part.view(np.uint8), full[:cap].view(np.uint8)), (r, free, cap)


def _drive_shards(name, cfg, G, shape, seed, need_exports=True):
    """the free-running frames of shape_cases.drive through oracle and shards, compare_union every 6th frame and after
    the last; the emitted clouds at the end"""
    o = _oracle(cfg, G)
    shards = _shards(cfg, G)
    S = 1 << cfg["p_n"]
    exported, eqs, cam = 0, [], None
    try:
        for t, depth, cloud, pos, q, mv, remove in sc.drive(shape, PARAMS, N_FRAMES, seed, cfg=cfg):
            fr = (depth, cloud, pos, q, mv)
            o.update(*fr, remove)
            exported += run_frame(shards, fr, remove)
            cam = pos
            eqs.append(o.ring_state()["eq_steps"][2])
            if t % 6 == 5 or t == N_FRAMES - 1:
                compare_union(o, shards, t, S)
        assert exported > 0 or not need_exports, "no copy crossed a slab border"
        d = np.diff(eqs)
        assert (d > 0).any() and (d < 0).any(), eqs      # the ring moved both ways along z: the slabs' contents changed hands
        vo = o.voxels()
        assert (vo["occ"] > 0).any() and (vo["occ"] == 0).any() and (vo["occ"] < 0).any()
        _check_emitted(cfg, o, shards, cam)
    finally:
        _close(shards)


@pytest.mark.parametrize("name", shc.SHAPE_CASES)
def test_shape_cases_on_thin_shards(name):
    cfg = shc.config(name)
    # (A/4 is here for its 16-voxel shards: on 4^3 cells of 1 m a few dozen particles move in these frames, none across a plane)
    _drive_shards(name, cfg, shc.CASES[name]["G"], shc.shape_of(name), seed=17, need_exports=name != "A/4")


def test_small_camera_shards_own_only_ck_padding():
    """T0 seen by a 48 x 40 camera at G = 32: the ck chunks of shards 30 and 31 lie wholly beyond the image"""
    name = "T0cam/32"
    cfg = shc.config(name)
    G = shc.CASES[name]["G"]
    assert shc.ck_empty_shards(cfg, G) == (30, 31)
    _drive_shards(name, cfg, G, None, seed=19)


@pytest.mark.parametrize("mode", ["scan", "lists", "all_dense"])
@pytest.mark.parametrize("name", shc.SWEEP_CASES)
def test_non_incremental_sweeps_on_thin_shards(name, mode):
    """every shard holds its slice of one random dense state (same stamps, same ring), every frame ends in a
    non-incremental sweep; in all-dense mode a shard hints whole 512-voxel groups only"""
    cfg = shc.config(name)
    G = shc.CASES[name]["G"]
    S = 1 << cfg["p_n"]
    o = _oracle(cfg, G)
    shards = _shards(cfg, G)
    n = shc.v_count(cfg, G)
    try:
        if mode == "all_dense":
            st = random_state(cfg, 7, run=8, kinds=(0.0, 0.0, 1.0))
        else:
            st = random_state(cfg, 5, run=8 if mode == "lists" else 1)
            for s in shards:
                s.m.force_sweep_lists(1 if mode == "lists" else 0)
        (sx, sy, sz), ring = stamps_for(o)
        o.load_state(st)
        o.set_stamps(sx, sy, sz)
        o.set_ring_state(ring)
        for r, s in enumerate(shards):
            s.m.load_state({k: v[r * n * S:(r + 1) * n * S] for k, v in st.items()})
            s.m.set_stamps(sx, sy, sz)
            s.m.set_ring_state(ring)
        hints, seen = [], set()
        for t, depth, cloud, pos, q, mv, remove in sc.drive(shc.shape_of(name), PARAMS, 4, seed=23):
            o.set_params(PARAMS)     # every frame ends in a non-incremental sweep
            for s in shards:
                s.m.set_params(PARAMS)
            fr = (depth, cloud, pos, q, mv)
            o.update(*fr, remove)
            run_frame(shards, fr, remove)
            compare_union(o, shards, t, S)
            hints.append([s.m.hinted_groups() for s in shards])
            seen |= set(np.sign(o.voxels()["occ"]).tolist())
        assert seen == {-1, 0, 1}, seen
        if mode == "all_dense":
            for h in hints[0]:
                assert (h == 0) if n < 512 else (0 < h <= n // 512), (hints[0], n)
    finally:
        _close(shards)


# ---- an object of more members than one shard has slots, moved across the ring's z wrap
def _big_frame(cfg, ring):
    depth = np.full((cfg["height"], cfg["width"]), np.nan, np.float32)
    cloud = np.zeros(cfg["height"] * cfg["width"], synth.LABELED_POINT)
    return (depth, cloud, np.array(ring["last_pos"], np.float32), synth.yaw_quat(0.0).astype(np.float32), shc.big_move(cfg, ring))


def _big_oracle(cfg, G, st, ring, fr):
    o = _oracle(cfg, G)
    o.load_state(st)
    o.set_ring_state(ring)
    o.update(*fr)
    return o


def _big_shards(cfg, G, st, ring, halo_cap):
    shards = _shards(cfg, G, halo_cap)
    n = shc.v_count(cfg, G) * (1 << cfg["p_n"])
    for r, s in enumerate(shards):
        s.m.load_state({k: v[r * n:(r + 1) * n] for k, v in st.items()})
        s.m.set_ring_state(ring)
    return shards


def test_object_larger_than_a_shard_moves_across_the_wrap():
    """17920 members (more than the 16384 and 8192 slots of a T0 shard at G = 16 and 32) moved about 5 planes up z
    across the ring's wrap: the oracle, the unsharded map and G = 16 and 32 agree, every map moved all of them, and the
    copies went to shards two slabs away and more, and from shard G-1 round the wrap to shard 0's side"""
    cfg = shc.config("T0/32")
    S = 1 << cfg["p_n"]
    ring = shc.big_ring(cfg)
    st = shc.big_state(cfg, ring)
    fr = _big_frame(cfg, ring)
    n_members = int((st["owner"] == shc.BIG_TRACK).sum())
    assert n_members == 17920
    o, g = pu.make_pair(cfg, PARAMS, synth.noise_table())
    try:
        for m in (o, g):
            m.load_state(st)
            m.set_ring_state(ring)
        o.update(*fr)
        g.update(*fr, sync=True)
        rep = pu.compare_maps(o, g, S, check_results=True)
        assert not rep, "\n".join(rep)
        assert o.stats()["n_moved"] == n_members and g.stats()["n_moved"] == n_members
    finally:
        g.close()
    for G in (16, 32):
        assert n_members > shc.v_count(cfg, G) * S
        og = _big_oracle(cfg, G, st, ring, fr)
        assert og.stats()["n_moved"] == n_members
        shards = _big_shards(cfg, G, st, ring, HALO_CAP)
        try:
            exported, hdr = run_frame(shards, fr, headers=True)
            compare_union(og, shards, 0, S)
            for s in shards:
                assert s.m.stats()["n_moved"] == n_members and s.m.stats()["halo_dropped"] == 0
            assert exported == int(hdr.sum()) > 0 and int(hdr.max()) <= HALO_CAP
            assert _far(hdr) > 0, hdr
            wrapped = [(s, d) for s, d in zip(*np.nonzero(hdr)) if d < s]   # moved up z, landed at a lower shard: round the wrap
            assert any(s == G - 1 for s, d in wrapped) and any(d == 0 for s, d in wrapped), wrapped
        finally:
            _close(shards)


def test_export_overflow_is_reported_exactly():
    """the same frame at G = 32 with 1024 records per export segment: each shard that dropped copies - and only such a
    shard - reports SDM_ERR_CAPACITY, naming the export segments, and counts exactly what it dropped; fresh shards whose
    segments hold the largest count take the frame and match the oracle"""
    cfg = shc.config("T0/32")
    G = 32
    S = 1 << cfg["p_n"]
    cap = 1024
    ring = shc.big_ring(cfg)
    st = shc.big_state(cfg, ring)
    fr = _big_frame(cfg, ring)
    shards = _big_shards(cfg, G, st, ring, cap)
    try:
        _, hdr = run_frame(shards, fr, headers=True, sync=False)
        dropped = np.maximum(hdr - cap, 0).sum(axis=1)
        assert (dropped > 0).any() and (dropped == 0).any(), hdr
        for r, s in enumerate(shards):
            if dropped[r] > 0:
                with pytest.raises(binding.SdmError, match="SDM_ERR_CAPACITY.*export segments"):
                    s.m.synchronize()
            else:
                s.m.synchronize()
            assert s.m.stats_unchecked()["halo_dropped"] == dropped[r], (r, hdr[r])
    finally:
        _close(shards)
    big = int(hdr.max())
    assert big > cap
    og = _big_oracle(cfg, G, st, ring, fr)
    shards = _big_shards(cfg, G, st, ring, big)
    try:
        _, hdr2 = run_frame(shards, fr, headers=True)
        assert np.array_equal(hdr2, hdr)
        compare_union(og, shards, 0, S)
        assert all(s.m.stats()["halo_dropped"] == 0 for s in shards)
    finally:
        _close(shards)
