"""sdm_world_match (include/sdm.h) against the grid model of tests/world_match_ref.py, bit for bit; the model is fed the
GPU's own world_bricks().

The archives are the ones tests/test_world_io_gpu.py builds: crafted maps of shape B archived by sdm_world_update, and
synthetic bricks imported into a map of shape A that serves as a handle.  Centre residues 0 / 1 / 7 (the window straddles 3
or 4 bricks per axis), bricks astride 0, a window at the end of the coordinate range, radius 0 and the largest radius, each
flag, duplicates, sources outside the archive, an archive with no brick near the sources, more source bricks than one
workgroup's run, the planted offset through world_match and world_align, device mode between canaries, scores == NULL,
n == 0, two runs with the same bytes, an archive that is left alone, a cross-check against world_region, the argument
checks."""
import ctypes as C
import itertools

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import world_io_ref as io
from tests import world_match_ref as mr
from tests import world_ref as wr
from tests import test_world_gpu as twg
from tests import test_world_io_gpu as tio

pytestmark = pytest.mark.gpu

INV = 1
MM = tio.MM
OTHER_LABEL = 1 << 24 | 11 << 16 | (MM + 1)
WORDS = np.concatenate([tio.WORDS, [tio.STATIC, OTHER_LABEL]]).astype(np.uint32)


def source(rng, coord):
    coord = np.asarray(coord, np.int64).reshape(-1, 3)
    return io.make_headers(coord), rng.choice(WORDS, size=(len(coord), 512))


def state(g):
    hdr, cells = g.world_bricks()
    return [g.world_info().tobytes(), hdr.tobytes(), cells.tobytes()]


def check(g, hdr, cells, mm=MM, flags=0, **kw):
    """world_match == the grid model over the GPU's own bricks, twice the same bytes, the archive untouched"""
    before = state(g)
    arch = g.world_bricks()
    res, scores = g.world_match(hdr, cells, static_only=bool(flags & wr.STATIC_ONLY), observed_only=bool(flags & wr.OBSERVED_ONLY), **kw)
    want, want_scores = mr.dense(hdr, cells, arch[0], arch[1], max_movable=mm, flags=flags, **kw)
    for name in binding.WORLD_MATCH_SCORE.names:
        bad = np.nonzero((scores[name] != want_scores[name]).reshape(len(scores), -1).any(axis=1))[0]
        assert not len(bad), (kw, name, len(bad), scores[bad[:3]], want_scores[bad[:3]])
    assert scores.tobytes() == want_scores.tobytes()
    assert res.tobytes() == want.tobytes(), (kw, res, want)
    again, again_scores = g.world_match(hdr, cells, static_only=bool(flags & wr.STATIC_ONLY), observed_only=bool(flags & wr.OBSERVED_ONLY), **kw)
    assert again.tobytes() == res.tobytes() and again_scores.tobytes() == scores.tobytes()
    assert state(g) == before
    return res, scores


def synthetic(rng, n_arch=40, lo=-3, hi=3):
    g = tio.handle()
    hdr, cells = source(rng, tio.random_coords(rng, n_arch, lo, hi))
    g.world_import(hdr, cells)
    return g


# ---- crafted archives of shape B: the centre's residues
@pytest.mark.parametrize("residue,sign", [(0, -1), (1, 1), (7, -1)])
def test_centre_residues_on_a_crafted_archive(residue, sign):
    cfg = sc.config("B")
    g = twg.crafted(cfg, twg.offset_steps(cfg, residue, sign), seed=60 + residue)
    g.world_update()
    hdr, cells = g.world_bricks()
    assert len(hdr) > 8
    rng = np.random.default_rng(residue)
    take = np.sort(rng.choice(len(hdr), min(len(hdr), 24), replace=False))
    mm = cfg["max_movable_track"]
    centre = ((residue + 1) % 8 - 1, residue, residue + 8)             # (the block is 4 cells wide in x: -1 for the residue 7 there)
    res, scores = check(g, hdr[take], cells[take], mm=mm, offset=centre, radius=(3, 3, 2))
    assert res["n_candidates"] == 245 and res["n_sources"] == len(take) and scores["n_oo"].sum() + scores["n_ff"].sum() > 0
    res, scores = check(g, hdr[take], cells[take], mm=mm, offset=(0, 0, 0), radius=(residue % 4, 1, 2))      # the archive against itself
    assert res["best_offset"].tolist() == [0, 0, 0] and scores[res["best"]]["n_oo"] == res["src_occupied"] == scores[res["best"]]["n_same"]
    assert scores[res["best"]]["n_of"] == 0 and scores[res["best"]]["n_fo"] == 0 and scores[res["best"]]["n_ff"] == res["src_free"]
    g.close()


def test_an_updated_archive_with_no_brick_near_the_sources():
    cfg = sc.config("B")
    g = twg.crafted(cfg, sc.crafted_steps(cfg), seed=5)
    g.world_update()
    info = g.world_info()
    rng = np.random.default_rng(1)
    far = info["bmax"].astype(np.int64) + 6
    hdr, cells = source(rng, far + np.array([[0, 0, 0], [1, 0, 0], [0, 2, 1]]))
    res, scores = check(g, hdr, cells, mm=cfg["max_movable_track"], offset=(1, 2, 3), radius=(2, 2, 1))
    assert not any(scores[f].any() for f in ("n_oo", "n_of", "n_fo", "n_ff", "n_same")) and res["best_offset"].tolist() == [1, 2, 3]
    assert res["src_occupied"] > 0 and res["best_score"] == 0 == res["runner_up"]
    g.close()


# ---- synthetic archives
@pytest.mark.parametrize("offset,radius", [((0, 0, 0), (1, 1, 1)), ((1, -1, 7), (2, 3, 1)), ((-7, 9, -16), (3, 0, 2)), ((5, 5, 5), (0, 0, 0)),
                                           ((-3, 2, 1), (0, 2, 0))])
def test_bricks_astride_zero(offset, radius):
    rng = np.random.default_rng(abs(sum(offset)) + 3)
    g = synthetic(rng)
    hdr, cells = source(rng, list(itertools.product((-1, 0), repeat=3)) + [[1, 0, -2]])      # every brick round the origin, and one more
    res, scores = check(g, hdr, cells, offset=offset, radius=radius)
    assert res["n_sources"] == 9 and (scores["n_same"] <= scores["n_oo"]).all() and scores["n_oo"].sum() > scores["n_same"].sum() > 0
    if radius == (0, 0, 0):
        assert res["n_candidates"] == 1 and res["best"] == 0 and res["runner_up"] == mr.INT64_MIN
    g.close()


@pytest.mark.parametrize("flags", wr.ALL_FLAGS)
def test_each_flag(flags):
    rng = np.random.default_rng(20 + flags)
    g = synthetic(rng, 30, -2, 2)
    hdr, cells = source(rng, tio.random_coords(rng, 6, -2, 1))
    res, _ = check(g, hdr, cells, flags=flags, offset=(2, -1, 3), radius=(1, 2, 1))
    plain, _ = g.world_match(hdr, cells, offset=(2, -1, 3), radius=(1, 2, 1))
    assert (res["src_occupied"] < plain["src_occupied"]) == bool(flags) and res["src_free"] == plain["src_free"]
    g.close()


def test_of_duplicated_sources_the_lowest_index_counts():
    rng = np.random.default_rng(31)
    g = synthetic(rng, 20, -2, 2)
    hdr, cells = source(rng, [[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0], [-1, -1, -1]])
    res, scores = check(g, hdr, cells, offset=(1, 1, 1), radius=(2, 1, 1))
    first, first_scores = g.world_match(hdr[[0, 1, 5]], cells[[0, 1, 5]], offset=(1, 1, 1), radius=(2, 1, 1))
    assert res.tobytes() == first.tobytes() and scores.tobytes() == first_scores.tobytes() and res["n_sources"] == 3
    g.close()


def test_sources_outside_the_archive_and_no_sources():
    rng = np.random.default_rng(32)
    g = synthetic(rng, 8, -1, 1)
    hdr, cells = source(rng, [[6, 6, 6], [7, 6, 6], [-9, 0, 0]])
    for h, c in ((hdr, cells), (hdr[:0], cells[:0])):
        res, scores = check(g, h, c, offset=(-2, 0, 2), radius=(2, 2, 2))
        assert not scores["n_oo"].any() and not scores["n_ff"].any() and res["best"] == 62 and res["best_offset"].tolist() == [-2, 0, 2]
        assert res["best_score"] == 0 == res["runner_up"] and res["n_sources"] == len(h)
    only, none = g.world_match(hdr, cells, radius=(1, 1, 1), scores=False)       # scores == NULL
    assert none is None and only.tobytes() == g.world_match(hdr, cells, radius=(1, 1, 1))[0].tobytes()
    g.close()


def test_a_window_at_the_end_of_the_coordinate_range():
    g = tio.handle()
    rng = np.random.default_rng(33)
    hdr, cells = source(rng, [[32767, 0, -32768], [32766, 0, -32768], [32767, 1, -32767]])
    g.world_import(hdr, cells)
    res, scores = check(g, hdr[:2], cells[:2], offset=(1, 0, -1), radius=(2, 1, 2))      # cells beyond the range read unknown
    assert scores["n_oo"].sum() > 0
    res, scores = check(g, hdr, cells, offset=(0, 0, 0), radius=(8, 0, 8))
    assert res["best_offset"].tolist() == [0, 0, 0] and scores[res["best"]]["n_oo"] == res["src_occupied"]
    g.close()


def test_the_largest_radius():
    rng = np.random.default_rng(34)
    g = synthetic(rng, 60, -3, 3)
    hdr, cells = source(rng, tio.random_coords(rng, 20, -2, 2))
    res, scores = check(g, hdr, cells, offset=(3, -5, 1), radius=(8, 8, 8))
    assert res["n_candidates"] == 17 ** 3 == len(scores) and scores["n_oo"].min() < scores["n_oo"].max()
    g.close()


def test_more_single_cell_bricks_than_one_run_of_workgroups():
    rng = np.random.default_rng(35)
    g = synthetic(rng, 300, -7, 7)
    coord = np.array(list(itertools.product(range(-6, 7), repeat=3)))              # 2197 sources: three to a workgroup
    hdr = io.make_headers(coord[rng.permutation(len(coord))])
    cells = np.full((len(hdr), 512), wr.UNKNOWN, np.uint32)
    cells[np.arange(len(hdr)), rng.integers(0, 512, len(hdr))] = rng.choice(WORDS[2:], len(hdr))
    res, scores = check(g, hdr, cells, offset=(1, 0, -1), radius=(1, 1, 1))
    assert res["n_sources"] == 2197 and res["src_occupied"] + res["src_free"] == 2197 and scores["n_oo"].sum() > 0
    g.close()


# ---- the planted offset
def test_the_planted_offset_is_recovered():
    arch = mr.blob_scene()
    hdr, cells = mr.shifted_copy(arch[0], arch[1], mr.PLANTED)
    g = tio.handle()
    g.world_import(*arch)
    res, scores = check(g, hdr, cells, mm=MM, offset=(0, 0, 0), radius=(4, 4, 2))
    best = scores[res["best"]]
    assert res["best_offset"].tolist() == list(mr.PLANTED) and res["runner_up"] < res["best_score"]
    assert best["n_of"] == 0 and best["n_fo"] == 0 and best["n_oo"] == res["src_occupied"]
    s = mr.score_of(scores, binding.WORLD_MATCH_WEIGHTS)
    assert (s == s.max()).sum() == 1
    offset, score, runner_up = g.world_align(hdr, cells, offset=(0, 0, 0), search=(12, 12, 4))     # (test_world_match_ref.py: nothing else comes near)
    assert offset.tolist() == list(mr.PLANTED) and score == res["best_score"] and runner_up < score
    before = state(g)                                      # ... and the import under it puts every cell back
    g.world_import(hdr, cells, offset=offset)
    assert state(g)[1:] == before[1:]
    g.close()


# ---- device mode
def test_device_mode_gives_what_host_mode_gives():
    rng = np.random.default_rng(36)
    g = synthetic(rng, 40, -3, 3)
    hdr, cells = source(rng, tio.random_coords(rng, 30, -3, 3))
    pad = 256

    def padded(raw):
        buf = np.full(len(raw) + 2 * pad, 0xA5, np.uint8)
        buf[pad:pad + len(raw)] = raw
        return g.device_put(buf), buf

    for offset, radius in (((1, 2, 3), (2, 2, 1)), ((-4, 0, 7), (4, 3, 2)), ((0, 0, 0), (1, 0, 0))):
        want, want_scores = g.world_match(hdr, cells, offset=offset, radius=radius)
        d_hdr, b_hdr = padded(np.frombuffer(hdr.tobytes(), np.uint8))
        d_cells, b_cells = padded(np.frombuffer(cells.tobytes(), np.uint8))
        d_scores, b_scores = padded(np.full(want_scores.nbytes, 0x5A, np.uint8))
        d_res, b_res = padded(np.full(want.nbytes, 0x5A, np.uint8))
        before = state(g)
        for with_scores in (True, False, True):            # (the work arrays are kept; the last call fills the records again)
            assert g.world_match(d_hdr + pad, d_cells + pad, offset=offset, radius=radius, on_device=True, n=len(hdr),
                                 scores=d_scores + pad if with_scores else None, result=d_res + pad) is None
        g.synchronize()
        got_scores, got_res = g.device_download(d_scores, len(b_scores)), g.device_download(d_res, len(b_res))
        assert got_scores[pad:-pad].tobytes() == want_scores.tobytes() and got_res[pad:-pad].tobytes() == want.tobytes()
        for got in (got_scores, got_res):
            assert (got[:pad] == 0xA5).all() and (got[-pad:] == 0xA5).all()
        assert np.array_equal(g.device_download(d_hdr, len(b_hdr)), b_hdr) and np.array_equal(g.device_download(d_cells, len(b_cells)), b_cells)
        assert state(g) == before
        for p in (d_hdr, d_cells, d_scores, d_res):
            g.device_free(p)
    d_res, b_res = padded(np.full(binding.WORLD_MATCH_RESULT.itemsize, 0x5A, np.uint8))       # n == 0 on the device
    g.world_match(0, 0, offset=(4, 4, 4), radius=(1, 1, 0), on_device=True, n=0, scores=None, result=d_res + pad)
    g.synchronize()
    got = g.device_download(d_res + pad, binding.WORLD_MATCH_RESULT.itemsize).view(binding.WORLD_MATCH_RESULT)[0]
    assert got.tobytes() == g.world_match(hdr[:0], cells[:0], offset=(4, 4, 4), radius=(1, 1, 0))[0].tobytes() and got["best"] == 4
    g.device_free(d_res)
    g.close()


# ---- an independent cross-check
def test_one_candidate_against_world_region():
    rng = np.random.default_rng(37)
    g = synthetic(rng, 40, -2, 2)
    hdr, cells = source(rng, tio.random_coords(rng, 10, -2, 2))
    res, scores = g.world_match(hdr, cells, offset=(2, -3, 1), radius=(2, 2, 1))
    k = 41
    lo, size = np.array([-16, -16, -16]), np.array([32, 32, 32])
    mine = np.full((32, 32, 32), wr.UNKNOWN, np.uint32)
    for i, b in enumerate(io.coords(hdr)):
        at = np.array(b) * 8 - lo
        mine[at[2]:at[2] + 8, at[1]:at[1] + 8, at[0]:at[0] + 8] = cells[i].reshape(8, 8, 8)
    theirs = g.world_region(lo + scores[k]["offset"], size)
    pairs = ((wr.occ_of(mine) >= 0) & (wr.occ_of(theirs) >= 0)).sum()
    assert pairs > 0 and pairs == int(scores[k]["n_oo"]) + int(scores[k]["n_of"]) + int(scores[k]["n_fo"]) + int(scores[k]["n_ff"])
    assert int(scores[k]["n_oo"]) == ((wr.occ_of(mine) >= 1) & (wr.occ_of(theirs) >= 1)).sum()
    g.close()


# ---- the argument checks
def test_argument_errors():
    g = tio.handle()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o, res = np.zeros(1, binding.WORLD_MATCH_OPTIONS), np.zeros(1, binding.WORLD_MATCH_RESULT)
    hdr, cells = io.make_headers([[0, 0, 0]]), np.zeros((1, 512), np.uint32)
    call = lambda *a: L.sdm_world_match(h, *a)  # noqa: E731
    assert call(vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == INV and b"sdm_world_update first" in L.sdm_last_error()   # no archive yet
    assert call(vp(o), None, None, 0, None, vp(res)) == INV
    g.world_import(hdr, cells)
    assert call(vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == 0 and call(vp(o), None, None, 0, None, vp(res)) == 0
    assert L.sdm_world_match(None, vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == INV
    assert call(None, vp(hdr), vp(cells), 1, None, vp(res)) == INV and call(vp(o), vp(hdr), vp(cells), 1, None, None) == INV
    assert call(vp(o), None, vp(cells), 1, None, vp(res)) == INV and call(vp(o), vp(hdr), None, 1, None, vp(res)) == INV
    assert call(vp(o), vp(hdr), vp(cells), -1, None, vp(res)) == INV and call(vp(o), vp(hdr), vp(cells), (1 << 21) + 1, None, vp(res)) == INV
    for flags in (0x04, 0x08, 0x10, 0x40, 1 << 31):
        o["flags"] = flags
        assert call(vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == INV and b"flag" in L.sdm_last_error()
    o["flags"] = 0
    for k in range(2):
        o["pad"][0, k] = 1
        assert call(vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == INV and b"pad" in L.sdm_last_error()
        o["pad"][0, k] = 0
    for a in range(3):
        for bad in (-1, 9, 1 << 30):
            o["radius"][0, a] = bad
            assert call(vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == INV and b"radius" in L.sdm_last_error()
        o["radius"][0, a] = 8
        for bad in ((1 << 19) + 1, -(1 << 19) - 1, -(1 << 31)):
            o["cell_offset"][0, a] = bad
            assert call(vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == INV and b"cell_offset" in L.sdm_last_error()
        o["cell_offset"][0, a] = (1 << 19) if a else -(1 << 19)
    assert call(vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == 0 and res[0]["n_candidates"] == 17 ** 3      # the largest everything
    g.world_clear()
    assert call(vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == INV
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], tio.PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert L.sdm_world_match(shard.h, vp(o), vp(hdr), vp(cells), 1, None, vp(res)) == INV and b"Z-slab shard" in L.sdm_last_error()
    shard.close()
