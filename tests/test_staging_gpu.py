"""The host-mode staging of the batched calls (sdm_query_points / sdm_query_segments, sdm_query_views, sdm_reach_paths)
driven through more than one chunk.  The property is split consistency: one host-mode call over the whole batch returns,
byte for byte, what host-mode calls over pieces that each fit in one chunk return, and what the same batch returns in
device mode.  The kernels are deterministic and the other GPU tests tie them to their NumPy restatements, so the GPU is
only compared with itself here.  The chunk sizes are restated from csrc/ (QUERY_CHUNK and VIEW_CHUNK_RAYS = 2^20, the
paths' 16 MiB of staged rows); the map is shape case "B" (4 x 32 x 64 cells, V = 8192) with the random block."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests.test_frontiers_gpu import crafted_map, pattern_block

pytestmark = pytest.mark.gpu

CHUNK = 1 << 20                       # queries.hip QUERY_CHUNK, views.hip VIEW_CHUNK_RAYS, reach.hip's CHUNK
N_QUERIES = CHUNK + 3                 # pieces [0, 2^20) and the last 3
N_RAYS, N_VIEWS = 65536, 17           # a chunk is max(1, 2^20 / n_rays) = 16 whole views: pieces of 16 and 1
V = 8192
N_GOALS, MAX_LEN = 513, V             # a staged row is min(max_len, V) cells, a chunk min(2^20, 16 MiB / (4 * row)) = 512 paths
FILL = 0xA5A5A5A5
assert max(1, CHUNK // N_RAYS) == 16 and min(CHUNK, (16 << 20) // (4 * min(MAX_LEN, V))) == 512
_MAP = []


def the_map():
    if not _MAP:
        _MAP.append(crafted_map("B", pattern_block("B", "random")))
        assert _MAP[0][1].V == V
    return _MAP[0]


def bounds(cfg, geo):
    size = np.float32(cfg["voxel_size"])
    lo = geo.center + geo.pmin
    return size, lo, lo + geo.N.astype(np.float32) * size


def points_round(cfg, geo, n, seed):
    """n points in and two cells round the map, NaN and infinity among the last ones"""
    size, lo, hi = bounds(cfg, geo)
    p = np.random.default_rng(seed).uniform(lo - 2 * size, hi + 2 * size, (n, 3)).astype(np.float32)
    p[-2:] = [[np.nan, 0, 0], [0, np.inf, 0]]
    return p


def test_points_and_segments_over_two_chunks():
    cfg, g, geo, vox = the_map()
    n = N_QUERIES
    a, b = points_round(cfg, geo, n, 1), points_round(cfg, geo, n, 2)[::-1].copy()
    res, idx = g.query_points(a, with_index=True)
    seg = g.query_segments(a, b)
    assert (idx != 0xFFFFFFFF).sum() > n // 4 and (idx == 0xFFFFFFFF).sum() > n // 4 and (seg["cells"] > 0).sum() > n // 4
    # the pieces, each one chunk
    for lo, hi in ((0, CHUNK), (CHUNK, n)):
        r, i = g.query_points(a[lo:hi], with_index=True)
        assert r.tobytes() == res[lo:hi].tobytes() and i.tobytes() == idx[lo:hi].tobytes(), (lo, hi)
        assert g.query_segments(a[lo:hi], b[lo:hi]).tobytes() == seg[lo:hi].tobytes(), (lo, hi)
    # device mode
    ab = np.ascontiguousarray(np.concatenate([a, b], axis=1))
    d_a, d_ab = g.device_put(a), g.device_put(ab)
    sizes = (n * 8, n * 4, n * 16)
    outs = [g.device_alloc(s) for s in sizes]
    g.query_points(d_a, on_device=True, n=n, out=outs[0], voxel_out=outs[1])
    g.query_segments(d_ab, on_device=True, n=n, out=outs[2])
    g.synchronize()
    for ptr, s, want in zip(outs, sizes, (res, idx, seg)):
        assert g.device_download(ptr, s).tobytes() == want.tobytes()
    for ptr in [d_a, d_ab] + outs:
        g.device_free(ptr)


def some_views(cfg, geo, n, seed):
    """n views in and just outside the map, turned every way, ranges of up to the map's length"""
    size, lo, hi = bounds(cfg, geo)
    rng = np.random.default_rng(seed)
    views = np.zeros(n, binding.VIEW)
    views["pos"] = rng.uniform(lo - size, hi + size, (n, 3)).astype(np.float32)
    q = rng.normal(size=(n, 4))
    views["q"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    views["range"] = rng.uniform(0.2, 1.0, n).astype(np.float32) * np.float32((hi - lo).max())
    views["pos"][[0, n - 1]] = (lo + hi) / 2    # the first and the last view from the middle of the map, whatever the draw
    return views


def unit_rays(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def test_views_over_two_chunks():
    cfg, g, geo, vox = the_map()
    views, dirs = some_views(cfg, geo, N_VIEWS, 3), unit_rays(N_RAYS, 4)
    gain, rays, unk = g.query_views(views, dirs, with_rays=True)
    assert (gain["rays_in_map"] > 0).sum() >= 9 and gain["rays_in_map"][16] > 0 and gain["n_unknown"].sum() > 0 and gain["rays_hit"].sum() > 0
    assert g.query_views(views, dirs).tobytes() == gain.tobytes()    # without the per-ray outputs
    for lo, hi in ((0, 16), (16, 17)):
        part = g.query_views(views[lo:hi], dirs, with_rays=True)
        for x, y in zip(part, (gain, rays, unk)):
            assert x.tobytes() == y[lo:hi].tobytes(), (lo, hi)
        assert g.query_views(views[lo:hi], dirs).tobytes() == gain[lo:hi].tobytes(), (lo, hi)
    # device mode
    d_views, d_dirs = g.device_put(views), g.device_put(dirs)
    sizes = (N_VIEWS * 40, N_VIEWS * N_RAYS * 16, N_VIEWS * N_RAYS * 4)
    outs = [g.device_alloc(s) for s in sizes]
    g.query_views(d_views, d_dirs, on_device=True, n_views=N_VIEWS, n_rays=N_RAYS, out=outs[0], rays_out=outs[1], ray_unknown_out=outs[2])
    g.synchronize()
    for ptr, s, want in zip(outs, sizes, (gain, rays, unk)):
        assert g.device_download(ptr, s).tobytes() == want.tobytes()
    g.query_views(d_views, d_dirs, on_device=True, n_views=N_VIEWS, n_rays=N_RAYS, out=outs[0])
    g.synchronize()
    assert g.device_download(outs[0], sizes[0]).tobytes() == gain.tobytes()
    for ptr in [d_views, d_dirs] + outs:
        g.device_free(ptr)


def build_reach(cfg, g):
    """the field from one start cell in the free half of the block (z >= 32) -> the start's cell word"""
    start = 1 | (16 << cfg["x_n"]) | (48 << (cfg["x_n"] + cfg["y_n"]))
    g.reach_update(start_cells=[start])
    return start


def used_cells(rows, lens):
    """the first min(len, max_len) cells of every row: what the call wrote (the rest of a row is the caller's fill)"""
    keep = np.arange(rows.shape[1])[None, :] < lens[:, None]
    return np.where(keep, rows, 0)


def test_paths_over_two_chunks():
    cfg, g, geo, vox = the_map()
    build_reach(cfg, g)
    goals = points_round(cfg, geo, N_GOALS, 5)
    rows, lens = g.reach_paths(xyz=goals, max_len=MAX_LEN, fill=FILL)
    assert (lens == 0).sum() >= 16 and lens[-1] == 0 and (lens[:512] > 1).sum() >= 16 and 0 < lens.max() < MAX_LEN
    assert (rows[~(np.arange(MAX_LEN)[None, :] < lens[:, None])] == FILL).all()
    for lo, hi in ((0, 512), (512, 513)):
        r, n = g.reach_paths(xyz=goals[lo:hi], max_len=MAX_LEN, fill=FILL)
        assert n.tobytes() == lens[lo:hi].tobytes(), (lo, hi)
        assert np.array_equal(used_cells(r, n), used_cells(rows[lo:hi], lens[lo:hi])), (lo, hi)
    # the last goal of a batch of 513 with a path: the second chunk copies a row out too
    again = np.concatenate([goals[1:], goals[int(np.argmax(lens))][None]])
    r, n = g.reach_paths(xyz=again, max_len=MAX_LEN, fill=FILL)
    assert n[-1] == lens.max() and np.array_equal(r[-1], rows[int(np.argmax(lens))]) and np.array_equal(used_cells(r[:-1], n[:-1]), used_cells(rows[1:], lens[1:]))
    # device mode
    d_goals, d_rows, d_lens = g.device_put(goals), g.device_put(np.full((N_GOALS, MAX_LEN), FILL, np.uint32)), g.device_alloc(N_GOALS * 4)
    g.reach_paths(xyz=d_goals, n=N_GOALS, max_len=MAX_LEN, on_device=True, cells_out=d_rows, len_out=d_lens)
    g.synchronize()
    assert g.device_download(d_lens, N_GOALS * 4, np.int32).tobytes() == lens.tobytes()
    dev_rows = g.device_download(d_rows, N_GOALS * MAX_LEN * 4, np.uint32).reshape(N_GOALS, MAX_LEN)
    assert np.array_equal(used_cells(dev_rows, lens), used_cells(rows, lens))
    for ptr in (d_goals, d_rows, d_lens):
        g.device_free(ptr)


def test_one_staging_area_under_three_layouts():
    """a fresh map, so that the staging area grows within this test: a 5-point query, the 17 views, the 513 paths and the
    5-point query again - the area laid out three ways, every later call over the stale contents of the one before"""
    cfg, g, geo, vox = crafted_map("B", pattern_block("B", "random"))
    build_reach(cfg, g)
    pts = points_round(cfg, geo, 5, 6)
    first = g.query_points(pts, with_index=True)
    views, dirs = some_views(cfg, geo, N_VIEWS, 3), unit_rays(N_RAYS, 4)
    got_views = g.query_views(views, dirs, with_rays=True)
    goals = points_round(cfg, geo, N_GOALS, 5)
    rows, lens = g.reach_paths(xyz=goals, max_len=MAX_LEN, fill=FILL)
    last = g.query_points(pts, with_index=True)
    assert last[0].tobytes() == first[0].tobytes() and last[1].tobytes() == first[1].tobytes()
    assert (first[1] != 0xFFFFFFFF).any()
    # ... and the calls in between returned what they return on the shared map, whose area grew in another order
    _, g2, _, _ = the_map()
    build_reach(cfg, g2)
    for x, y in zip(got_views, g2.query_views(views, dirs, with_rays=True)):
        assert x.tobytes() == y.tobytes()
    rows2, lens2 = g2.reach_paths(xyz=goals, max_len=MAX_LEN, fill=FILL)
    assert rows.tobytes() == rows2.tobytes() and lens.tobytes() == lens2.tobytes()
    g.close()
