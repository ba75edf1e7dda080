"""sdm_query_world_segments / sdm_query_world_views (include/sdm.h) against tests/world_rays_ref.py's BrickWalk, byte for
byte.  The model is fed with what world_bricks() of the same map returns.

The archive needs a map only as a handle: every case but the last two feeds the hand-written bricks of
tests/world_rays_cases.py to world_import on a fresh map of shape A (voxel_size 1).  The crafted cases with their closed
forms; the random archive under every flag in host and device mode, with canaries round the device outputs at an 8-byte
offset; rays_out against the segment query; batching through the hook; the pool left zero; two reaches in a row; no side
effects; retain and clear; the argument checks; then two tests on frames: agreement with the block's segment query, and the
exploration loop beyond the block."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import test_world_gpu as twg
from tests import views_ref as vr
from tests import world_rays_cases as rc
from tests import world_rays_ref as rr
from tests.test_ground_gpu import _cells
from tests.test_world_rays_ref import check_want

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV = 1
CAN = 0xA5
F = np.float32
HIT, GAIN = binding.WORLD_SEGMENT_HIT, binding.VIEW_GAIN
SEGMENTS, VIEWS = rc.segment_cases(), rc.view_cases()


def world_of(arch):
    g = binding.SdmMap(rc.CFG, PARAMS, synth.noise_table())
    g.world_import(arch[0], arch[1])
    return g


def model_of(g, size=rc.SIZE, max_movable=rc.MM):
    hdr, cells = g.world_bricks()
    return rr.BrickWalk(hdr, cells, size, max_movable)


def device_segments(g, a, b, **kw):
    """device mode, the output 8 bytes into a buffer of canaries"""
    ab = np.ascontiguousarray(np.concatenate([np.asarray(a, F).reshape(-1, 3), np.asarray(b, F).reshape(-1, 3)], axis=1))
    n = len(ab)
    d_in, d_out = g.device_put(ab), g.device_put(np.full(n * 32 + 16, CAN, np.uint8))
    g.query_world_segments(d_in, on_device=True, n=n, out=d_out + 8, **kw)
    g.synchronize()
    raw = g.device_download(d_out, n * 32 + 16)
    g.device_free(d_in), g.device_free(d_out)
    assert (raw[:8] == CAN).all() and (raw[-8:] == CAN).all()
    return raw[8:-8].view(HIT)


def device_views(g, views, dirs, reach, with_rays=True, **kw):
    views, dirs = np.ascontiguousarray(views, binding.VIEW).reshape(-1), np.ascontiguousarray(dirs, F).reshape(-1, 3)
    nv, nr = len(views), len(dirs)
    d_v, d_d = g.device_put(views), g.device_put(dirs)
    d_g, d_r = g.device_put(np.full(nv * 40 + 16, CAN, np.uint8)), g.device_put(np.full(nv * nr * 32 + 16, CAN, np.uint8))
    g.query_world_views(d_v, d_d, reach, on_device=True, n_views=nv, n_rays=nr, out=d_g + 8, rays_out=(d_r + 8) if with_rays else None, **kw)
    g.synchronize()
    raw_g, raw_r = g.device_download(d_g, nv * 40 + 16), g.device_download(d_r, nv * nr * 32 + 16)
    for p in (d_v, d_d, d_g, d_r):
        g.device_free(p)
    assert (raw_g[:8] == CAN).all() and (raw_g[-8:] == CAN).all() and (raw_r[:8] == CAN).all() and (raw_r[-8:] == CAN).all()
    if not with_rays:
        assert (raw_r == CAN).all()
    return raw_g[8:-8].view(GAIN), raw_r[8:-8].view(HIT).reshape(nv, nr)


# ---- the crafted cases
@pytest.mark.parametrize("name", sorted(SEGMENTS))
def test_crafted_segments(name):
    c = SEGMENTS[name]
    g = world_of(c["arch"])
    want = model_of(g).segments(c["a"][None], c["b"][None], **c["kw"])
    host = g.query_world_segments(c["a"][None], c["b"][None], **c["kw"])
    print(name, host, want)
    assert host.tobytes() == want.tobytes()
    check_want(name, host[0], c["want"])
    assert device_segments(g, c["a"][None], c["b"][None], **c["kw"]).tobytes() == want.tobytes()
    g.close()


@pytest.mark.parametrize("name", sorted(VIEWS))
def test_crafted_views(name):
    c = VIEWS[name]
    g = world_of(c["arch"])
    want_g, want_r = model_of(g).views(c["views"], c["dirs"], c["reach"], **c["kw"])
    gain, rays = g.query_world_views(c["views"], c["dirs"], c["reach"], with_rays=True, **c["kw"])
    print(name, gain, want_g)
    assert gain.tobytes() == want_g.tobytes() and rays.tobytes() == want_r.tobytes()
    check_want(name, gain[0], c["want"])
    assert g.query_world_views(c["views"], c["dirs"], c["reach"], **c["kw"]).tobytes() == want_g.tobytes()     # without rays_out
    dev_g, dev_r = device_views(g, c["views"], c["dirs"], c["reach"], **c["kw"])
    assert dev_g.tobytes() == want_g.tobytes() and dev_r.tobytes() == want_r.tobytes()
    g.close()


# ---- the random archive: 512 segments under every flag, 12 views, host and device mode
RANDOM = {}


def random_world():
    """the map, the model and the model's answers, computed once and left unchanged"""
    if not RANDOM:
        g = world_of(rc.random_archive())
        RANDOM.update(g=g, ref=model_of(g), ab=rc.random_segments(), views=rc.random_views(), seg={}, view={})
    return RANDOM


def random_segments_want(kw):
    r = random_world()
    key = tuple(sorted(kw.items()))
    if key not in r["seg"]:
        r["seg"][key] = r["ref"].segments(*r["ab"], **kw)
    return r["seg"][key]


def random_views_want(reach, ignore_movable=False):
    r = random_world()
    if (reach, ignore_movable) not in r["view"]:
        r["view"][reach, ignore_movable] = r["ref"].views(r["views"], rc.PINHOLE, reach, ignore_movable=ignore_movable)
    return r["view"][reach, ignore_movable]


@pytest.mark.parametrize("unknown_blocks", (False, True))
@pytest.mark.parametrize("ignore_movable", (False, True))
def test_random_segments(unknown_blocks, ignore_movable):
    r, kw = random_world(), dict(unknown_blocks=unknown_blocks, ignore_movable=ignore_movable)
    want = random_segments_want(kw)
    host = r["g"].query_world_segments(*r["ab"], **kw)
    bad = np.flatnonzero(host != want)
    assert host.tobytes() == want.tobytes(), (bad[:5], host[bad[:5]], want[bad[:5]])
    assert device_segments(r["g"], *r["ab"], **kw).tobytes() == want.tobytes()


@pytest.mark.parametrize("reach,ignore_movable", ((20, False), (6, True)))
def test_random_views(reach, ignore_movable):
    r = random_world()
    want_g, want_r = random_views_want(reach, ignore_movable)
    gain, rays = r["g"].query_world_views(r["views"], rc.PINHOLE, reach, with_rays=True, ignore_movable=ignore_movable)
    print(gain, want_g)
    assert gain.tobytes() == want_g.tobytes() and rays.tobytes() == want_r.tobytes()
    dev_g, dev_r = device_views(r["g"], r["views"], rc.PINHOLE, reach, ignore_movable=ignore_movable)
    assert dev_g.tobytes() == want_g.tobytes() and dev_r.tobytes() == want_r.tobytes()
    dev_g, _ = device_views(r["g"], r["views"], rc.PINHOLE, reach, with_rays=False, ignore_movable=ignore_movable)
    assert dev_g.tobytes() == want_g.tobytes()


def test_rays_out_is_the_segment_query_where_the_window_holds_the_segment():
    r = random_world()
    for reach, ignore_movable in ((20, False), (6, True)):
        _, rays = r["g"].query_world_views(r["views"], rc.PINHOLE, reach, with_rays=True, ignore_movable=ignore_movable)
        a, b, given = vr.rays_of(r["views"], rc.PINHOLE)
        seg = r["g"].query_world_segments(a.reshape(-1, 3), b.reshape(-1, 3), ignore_movable=ignore_movable).reshape(rays.shape)
        inside = given & (np.abs(np.floor(b) - np.floor(a)).max(axis=2) <= reach)       # voxel_size 1: a position is its coordinate
        assert inside.sum() > (200 if reach == 20 else 20) and not inside.all()
        assert rays[inside].tobytes() == seg[inside].tobytes()
        assert (rays[~inside]["cells"] <= 3 * reach + 1).all()


# ---- batching through the hook, and the pool left all zero
def test_batches_give_equal_bytes_and_the_pool_is_left_zero():
    r = random_world()
    g = r["g"]
    want_g, want_r = random_views_want(20)
    other = VIEWS["several views"]
    try:
        for batch in (1, 2, 5, 0):
            g.set_world_view_batch(batch)
            gain, rays = g.query_world_views(r["views"], rc.PINHOLE, 20, with_rays=True)
            assert gain.tobytes() == want_g.tobytes() and rays.tobytes() == want_r.tobytes(), batch
            # a different set in between, then the same views again: a bit left set would hide a cell
            between = g.query_world_views(other["views"], other["dirs"], 9)
            again = g.query_world_views(r["views"], rc.PINHOLE, 20)
            assert again.tobytes() == want_g.tobytes(), batch
            assert between.tobytes() == g.query_world_views(other["views"], other["dirs"], 9).tobytes()
    finally:
        g.set_world_view_batch(0)


def test_a_smaller_reach_after_a_larger_one():
    """the larger window's masks are longer; the smaller one's lie over their zeroed words"""
    r = random_world()
    g = r["g"]
    big = g.query_world_views(r["views"], rc.PINHOLE, 40)
    assert g.query_world_views(r["views"], rc.PINHOLE, 6, ignore_movable=True).tobytes() == random_views_want(6, True)[0].tobytes()
    assert g.query_world_views(r["views"], rc.PINHOLE, 20).tobytes() == random_views_want(20)[0].tobytes()
    assert g.query_world_views(r["views"], rc.PINHOLE, 40).tobytes() == big.tobytes()
    assert (big["ray_cells"] >= random_views_want(20)[0]["ray_cells"]).all()
    # the largest reach: 16.7 MB a mask, four views in flight
    c = VIEWS["one ray, reach 20"]
    top = g.query_world_views(np.repeat(c["views"], 6), c["dirs"], binding.WORLD_VIEW_MAX_REACH)
    assert (top == top[0]).all() and top[0]["rays_in_map"] == 1


def test_no_side_effects_and_host_mode_writes_nothing_behind_its_results():
    r = random_world()
    g = r["g"]
    state = lambda: [a.tobytes() for a in g.world_bricks()] + [g.world_info().tobytes(), g.voxels().tobytes(), repr(g.ring_state())]  # noqa: E731
    before = state()
    a, b = r["ab"]
    g.query_world_segments(a, b, unknown_blocks=True)
    g.query_world_views(r["views"], rc.PINHOLE, 20, with_rays=True)
    assert state() == before
    L, h, vp = g.L, g.h, lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    ab = np.ascontiguousarray(np.concatenate([a, b], axis=1))
    out = np.full((len(ab) + 1) * 32, CAN, np.uint8)
    assert L.sdm_query_world_segments(h, vp(ab), len(ab), vp(out), 0) == 0
    assert (out[len(ab) * 32:] == CAN).all() and out[:len(ab) * 32].tobytes() == random_segments_want(dict(unknown_blocks=False, ignore_movable=False)).tobytes()
    assert L.sdm_query_world_segments(h, vp(ab), 0, vp(out), 0) == 0 and (out[len(ab) * 32:] == CAN).all()
    gain = np.full(40, CAN, np.uint8)
    assert L.sdm_query_world_views(h, vp(r["views"]), 0, vp(rc.PINHOLE), len(rc.PINHOLE), 4, vp(gain), None, 0) == 0 and (gain == CAN).all()


def test_queries_follow_retain_import_and_clear():
    """no snapshot: the queries see the archive as the last call before them left it"""
    g = world_of(rc.random_archive())
    a, b = rc.random_segments(128, seed=41)
    views = rc.random_views(3, seed=43)

    def check():
        ref = model_of(g)
        assert g.query_world_segments(a, b).tobytes() == ref.segments(a, b).tobytes()
        want_g, want_r = ref.views(views, rc.PINHOLE[::3], 12)
        gain, rays = g.query_world_views(views, rc.PINHOLE[::3], 12, with_rays=True)
        assert gain.tobytes() == want_g.tobytes() and rays.tobytes() == want_r.tobytes()
        return gain, rays

    full = check()
    assert g.world_retain(bmin=(1, -1, 0), bmax=(5, 5, 5)) > 0          # removes half the bricks and compacts the pool
    trimmed = check()
    assert trimmed[0].tobytes() != full[0].tobytes() and trimmed[1].tobytes() != full[1].tobytes()
    room = rc.room()
    g.world_import(room[0], room[1], offset=(3, 0, -5))
    check()
    g.world_clear()
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        g.query_world_segments(a, b)
    with pytest.raises(binding.SdmError, match="sdm_world_update first"):
        g.query_world_views(views, rc.PINHOLE, 12)
    g.world_import(room[0], room[1])                                    # the emptied archive filled again
    check()
    assert g.world_retain(bmin=(0, 0, 0), bmax=(-1, 0, 0)) == 27 and g.world_info()["n_bricks"] == 0
    empty = check()[0]                                                  # an archive without bricks: everything is unknown
    assert (empty["n_free"] == 0).all() and (empty["n_occupied"] == 0).all() and (empty["n_unknown"] > 0).all()
    g.close()


# ---- the argument checks
def test_argument_errors():
    g = binding.SdmMap(rc.CFG, PARAMS, synth.noise_table())
    L, h, vp = g.L, g.h, lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    ab, out = np.zeros((2, 6), F), np.zeros(2, HIT)
    views, dirs, gain, rays = np.zeros(2, binding.VIEW), np.zeros((3, 3), F), np.zeros(2, GAIN), np.zeros(6, HIT)
    segments = lambda *x: L.sdm_query_world_segments(h, *x)  # noqa: E731
    score = lambda *x: L.sdm_query_world_views(h, *x)  # noqa: E731
    # before any update or import
    assert segments(vp(ab), 2, vp(out), 0) == INV and b"sdm_world_update first" in L.sdm_last_error()
    assert score(vp(views), 2, vp(dirs), 3, 4, vp(gain), vp(rays), 0) == INV and b"sdm_world_update first" in L.sdm_last_error()
    room = rc.room()
    g.world_import(room[0], room[1])
    assert segments(vp(ab), 2, vp(out), 0) == 0 and score(vp(views), 2, vp(dirs), 3, 4, vp(gain), vp(rays), 0) == 0
    # segments
    assert segments(None, 2, vp(out), 0) == INV and segments(vp(ab), 2, None, 0) == INV and segments(vp(ab), -1, vp(out), 0) == INV
    for bad in (0x4, 0x8, 0x20, 0x80000000):
        assert segments(vp(ab), 2, vp(out), bad) == INV and b"flag" in L.sdm_last_error()
    assert segments(vp(ab), 2, vp(out), 0x2 | 0x10) == 0
    # views
    assert score(None, 2, vp(dirs), 3, 4, vp(gain), None, 0) == INV and score(vp(views), 2, None, 3, 4, vp(gain), None, 0) == INV
    assert score(vp(views), 2, vp(dirs), 3, 4, None, None, 0) == INV and score(vp(views), -1, vp(dirs), 3, 4, vp(gain), None, 0) == INV
    for n_rays in (0, -1, binding.VIEW_MAX_RAYS + 1):
        assert score(vp(views), 2, vp(dirs), n_rays, 4, vp(gain), None, 0) == INV and b"n_rays" in L.sdm_last_error()
    assert score(vp(views), 1 << 29, vp(dirs), 4, 4, vp(gain), None, 0) == INV
    for reach in (0, -3, binding.WORLD_VIEW_MAX_REACH + 1):
        assert score(vp(views), 2, vp(dirs), 3, reach, vp(gain), None, 0) == INV and b"reach_cells" in L.sdm_last_error()
    for bad in (0x2, 0x4, 0x8, 0x12):                                    # UNKNOWN_BLOCKS is refused here
        assert score(vp(views), 2, vp(dirs), 3, 4, vp(gain), None, bad) == INV and b"flag" in L.sdm_last_error()
    assert score(vp(views), 2, vp(dirs), 3, 4, vp(gain), None, 0x10) == 0
    assert score(vp(views), 0, vp(dirs), 3, 4, vp(gain), None, 0) == 0
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert L.sdm_query_world_segments(shard.h, vp(ab), 2, vp(out), 0) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_query_world_views(shard.h, vp(views), 2, vp(dirs), 3, 4, vp(gain), None, 0) == INV and b"Z-slab shard" in L.sdm_last_error()
    shard.close()


# ---- on frames 1: agreement with the block
def test_agreement_with_the_block():
    """after one world_update of an empty archive with no flags the archive holds the block: axis-aligned segments between
    cell centres inside the block get the same answer from the block's query and from the world's"""
    cfg = sc.config("B")
    N = twg.dims(cfg)
    steps = np.array(sc.crafted_steps(cfg), np.int64)
    g = twg.crafted(cfg, steps, seed=12)
    g.world_update()
    size = F(cfg["voxel_size"])
    g0 = steps - (N >> 1)                                # world cell of the block's cell (0, 0, 0)
    rng = np.random.default_rng(8)
    n = 300
    ca = np.stack([rng.integers(0, N[k], n) for k in range(3)], 1)
    cb = ca.copy()
    axis = rng.integers(0, 3, n)
    cb[np.arange(n), axis] = rng.integers(0, N[axis])
    centre = lambda c: ((c + g0).astype(F) + F(0.5)) * size  # noqa: E731
    a, b = centre(ca), centre(cb)
    for unknown_blocks in (False, True):
        block = g.query_segments(a, b, unknown_blocks=unknown_blocks)
        world = g.query_world_segments(a, b, unknown_blocks=unknown_blocks)
        hit = block["t"] >= 0
        assert 20 < hit.sum() < n - 20
        assert np.array_equal(world["t"] >= 0, hit) and np.array_equal(world["cells"], block["cells"]) and np.array_equal(world["t"], block["t"])
        for k in ("track", "label", "occ"):
            assert np.array_equal(world[k], block[k]), k
        # world cell = block cell + g0: the block's storage index of the world's hit cell is the block's hit voxel
        _, index = g.query_points(((world["cell"][hit]).astype(F) + F(0.5)) * size, with_index=True)
        assert np.array_equal(index, block["voxel"][hit])
        step = np.sign(cb - ca)[hit] * (world["cells"][hit] - 1)[:, None]
        assert np.array_equal(world["cell"][hit], (ca + g0)[hit] + step)
    assert world.tobytes() == model_of(g, size, cfg["max_movable_track"]).segments(a, b, unknown_blocks=True).tobytes()
    g.close()


# ---- on frames 2: the exploration loop beyond the block
def test_the_exploration_loop_beyond_the_block():
    """the drive of tests/test_world_esdf_gpu.py: the camera leaves what it archived.  A view at a world frontier cluster
    behind the block, looking away from it, is nothing to the block's view scoring and a gain to the world's; the legs of the
    world reach path to the cluster are free."""
    cfg = sc.config("B")
    N = twg.dims(cfg)
    size = F(cfg["voxel_size"])
    rng = np.random.default_rng(4)
    u = rng.random(tuple(N[::-1]))
    occ = np.zeros(tuple(N[::-1]), np.int8)
    occ[u < 0.03] = -1
    occ[u < 0.003] = 1
    drive = int(N[2]) // 4
    occ[int(N[2]) // 2 + drive - 3:int(N[2]) // 2 + drive + 4, int(N[1]) // 2 - 3:int(N[1]) // 2 + 3, :] = 0   # free where the camera will stand
    steps = np.array(sc.crafted_steps(cfg), np.int64)
    ring = sc.crafted_ring(cfg, steps)
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    n_occ = int((occ == 1).sum())
    g.load_state(sc.crafted_state(cfg, ring, _cells(occ == 1), _cells(occ == -1), tracks=np.full(n_occ, 65535), labels=np.full(n_occ, 8)))
    g.set_ring_state(ring)
    twg.blind_frame(g, cfg, ring["last_pos"])
    g.world_update()
    for _ in range(2):                                   # the camera drives off along z; what comes in is unobserved
        steps[2] += drive // 2
        twg.blind_frame(g, cfg, twg.cam_of(cfg, steps))
        g.world_update()
    cam = twg.cam_of(cfg, steps)
    g0 = steps - (N >> 1)                                # world cell of the block's cell (0, 0, 0)
    # where: the frontier clusters of the bricks that lie wholly behind the block
    info = g.world_info()
    behind = (int(g0[2]) >> 3) - 1
    assert info["bmin"][2] <= behind
    g.world_frontiers_update(box=(tuple(int(v) for v in info["bmin"]), (int(info["bmax"][0]), int(info["bmax"][1]), behind)), min_cells=4)
    clusters, _ = g.world_frontiers()
    assert len(clusters) > 0
    # how far: face-connected, so that a leg from cell centre to cell centre visits the two cells of the path only
    g.world_reach_update(starts=[cam], face_connected=True, through_unknown=True)
    reach = g.query_world_reach(cells=clusters["first_cell"])
    reached = np.flatnonzero(reach["cost"] != binding.REACH_NO_COST)
    assert len(reached) > 0
    k = reached[np.argmax(clusters["n_cells"][reached])]
    centroid = clusters["centroid"][k]
    assert centroid[2] < F(g0[2]) * size                 # outside the current block
    # how much would I learn there: a camera at the centroid looking away from the block (camera z = world -z)
    v = np.zeros(1, binding.VIEW)
    v["pos"], v["q"], v["range"] = centroid, (0.0, 1.0, 0.0, 0.0), 3.0
    dirs = rc.PINHOLE
    block = g.query_views(v, dirs)
    assert block["rays_in_map"][0] == 0 and block["n_unknown"][0] == 0
    want_g, want_r = model_of(g, size, cfg["max_movable_track"]).views(v, dirs, 16)
    gain, rays = g.query_world_views(v, dirs, 16, with_rays=True)
    print("gain beyond the block:", gain)
    assert gain.tobytes() == want_g.tobytes() and rays.tobytes() == want_r.tobytes()
    assert gain["n_unknown"][0] > 0 and gain["n_free"][0] > 0 and gain["rays_in_map"][0] == len(dirs)
    # is the way free: the path's legs
    goal = clusters["first_cell"][k][None]
    rows, lens = g.world_reach_paths(cells=goal, max_len=int(reach["cost"][k]) // binding.REACH_COST_PER_CELL + 1)
    path = rows[0, :lens[0]]
    assert lens[0] > 8 and path[0].tolist() == goal[0].tolist() and (np.abs(np.diff(path, axis=0)).sum(axis=1) == 1).all()
    centres = (path.astype(F) + F(0.5)) * size
    legs = g.query_world_segments(centres[:-1], centres[1:])
    assert (legs["t"] == -1.0).all() and (legs["cells"] == 2).all()
    g.close()
