"""tests/world_match_ref.py against itself: the grid model and the cell-by-cell model of sdm_world_match agree byte for byte
- all residues of the centre, bricks astride 0 and at negative coordinates, radius 0 and asymmetric radii, every flag set
with guessed and movable words, differing labels, duplicated sources, sources wholly outside the archive, the tie rule -
and the planted-offset scene the GPU tests rely on does what they need: the planted offset is the strict, unique maximum."""
import itertools

import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import world_io_ref as io
from tests import world_match_ref as mr
from tests import world_ref as wr

MM = 5
FREE, MOVING, STATIC, GUESS_MOVING, GUESS_STATIC = 0, 1 << 24 | 7 << 16 | 3, 1 << 24 | 8 << 16 | (MM + 1), 2 << 24 | 7 << 16 | MM, 2 << 24 | 9 << 16 | 65535
OTHER_LABEL = 1 << 24 | 11 << 16 | (MM + 1)
WORDS = np.array([wr.UNKNOWN, wr.UNKNOWN, wr.UNKNOWN, FREE, FREE, MOVING, STATIC, STATIC, GUESS_MOVING, GUESS_STATIC, OTHER_LABEL], np.uint32)


def bricks(rng, coord):
    coord = np.asarray(coord, np.int64).reshape(-1, 3)
    return io.make_headers(coord), rng.choice(WORDS, size=(len(coord), 512))


def some_coords(rng, n, lo, hi):
    box = np.array(list(itertools.product(range(lo, hi), repeat=3)))
    return box[rng.choice(len(box), n, replace=False)]


def both(hdr, cells, arch, **kw):
    d_res, d_sc = mr.dense(hdr, cells, arch[0], arch[1], **kw)
    n_res, n_sc = mr.naive(hdr, cells, mr.naive_archive(*arch), **kw)
    assert d_sc.tobytes() == n_sc.tobytes(), kw
    assert d_res.tobytes() == n_res.tobytes(), (kw, d_res, n_res)
    return d_res, d_sc


@pytest.mark.parametrize("residue", [0, 1, 7])
def test_every_residue_of_the_centre_astride_zero(residue):
    rng = np.random.default_rng(residue)
    arch = bricks(rng, some_coords(rng, 20, -2, 2))
    hdr, cells = bricks(rng, some_coords(rng, 4, -1, 1))
    for axis in range(3):
        offset = [0, 0, 0]
        offset[axis] = residue - 8 * (axis == 1)
        res, sc = both(hdr, cells, arch, offset=offset, radius=(1, 1, 1), max_movable=MM)
        assert res["n_candidates"] == 27 and res["n_sources"] == 4 and sc["n_oo"].sum() > 0 and sc["n_ff"].sum() > 0
        assert (sc["n_same"] <= sc["n_oo"]).all() and (sc["n_same"] < sc["n_oo"]).any() and sc["n_same"].sum() > 0


def test_radius_zero_and_asymmetric_radii():
    rng = np.random.default_rng(4)
    arch = bricks(rng, some_coords(rng, 30, -3, 1))
    hdr, cells = bricks(rng, some_coords(rng, 3, -2, 0))
    res, sc = both(hdr, cells, arch, offset=(-3, 2, 9), radius=(0, 0, 0), max_movable=MM)
    assert res["n_candidates"] == 1 and res["best"] == 0 and res["runner_up"] == mr.INT64_MIN and sc[0]["offset"].tolist() == [-3, 2, 9]
    res, sc = both(hdr, cells, arch, offset=(5, -7, 1), radius=(2, 0, 1), max_movable=MM)
    assert res["n_candidates"] == 15 and sc[0]["offset"].tolist() == [3, -7, 0] and sc[1]["offset"].tolist() == [4, -7, 0]
    assert sc[5]["offset"].tolist() == [3, -7, 1] and res["runner_up"] != mr.INT64_MIN


@pytest.mark.parametrize("flags", wr.ALL_FLAGS)
def test_flags_class_both_sides(flags):
    rng = np.random.default_rng(5)
    arch = bricks(rng, some_coords(rng, 8, -1, 1))
    hdr, cells = bricks(rng, some_coords(rng, 3, -1, 1))
    res, sc = both(hdr, cells, arch, offset=(1, 0, -1), radius=(1, 1, 0), max_movable=MM, flags=flags)
    occ, track = wr.occ_of(cells), cells & 0xFFFF
    gone = np.zeros(cells.shape, bool)
    if flags & wr.STATIC_ONLY:
        gone |= (occ >= 1) & (track >= 1) & (track <= MM)
    if flags & wr.OBSERVED_ONLY:
        gone |= occ == 2
    assert res["src_occupied"] == ((occ >= 1) & ~gone).sum() and res["src_free"] == (occ == 0).sum()
    plain, _ = mr.dense(hdr, cells, arch[0], arch[1], offset=(1, 0, -1), radius=(1, 1, 0), max_movable=MM)
    assert (res["src_occupied"] < plain["src_occupied"]) == bool(flags)


def test_of_duplicated_sources_the_lowest_index_counts():
    rng = np.random.default_rng(6)
    arch = bricks(rng, some_coords(rng, 8, -1, 1))
    hdr, cells = bricks(rng, [[0, 0, 0], [-1, 0, 0], [0, 0, 0], [-1, 0, 0], [0, 0, 0]])
    res, sc = both(hdr, cells, arch, radius=(1, 1, 1), max_movable=MM)
    want, want_sc = mr.dense(hdr[:2], cells[:2], arch[0], arch[1], radius=(1, 1, 1), max_movable=MM)
    assert res.tobytes() == want.tobytes() and sc.tobytes() == want_sc.tobytes() and res["n_sources"] == 2


def test_sources_outside_the_archive_and_no_sources_pick_the_centre():
    rng = np.random.default_rng(7)
    arch = bricks(rng, some_coords(rng, 8, -1, 1))
    hdr, cells = bricks(rng, [[5, 5, 5], [6, 5, 5]])
    for h, c in ((hdr, cells), (hdr[:0], cells[:0])):
        res, sc = both(h, c, arch, offset=(2, 2, 2), radius=(2, 1, 2), max_movable=MM)
        assert not sc["n_oo"].any() and not sc["n_ff"].any() and res["best_score"] == 0 and res["runner_up"] == 0
        assert res["best"] == (res["n_candidates"] - 1) // 2 and res["best_offset"].tolist() == [2, 2, 2]
    assert res["n_sources"] == 0 and res["src_occupied"] == 0


def test_ties_go_to_the_nearest_then_to_the_lowest_index():
    # one occupied source cell, two occupied archive cells at d = (-1, 0, 0) and d = (0, 0, 1): equal scores, equal distances,
    # the lower index wins; a third at d = (1, 1, 0) is further and loses; with it alone scoring, distance decides nothing
    cells = np.full((1, 512), wr.UNKNOWN, np.uint32)
    cells[0, 3 | 3 << 3 | 3 << 6] = STATIC
    hdr = io.make_headers([[0, 0, 0]])
    a_cells = np.full((1, 512), wr.UNKNOWN, np.uint32)
    for d in ((-1, 0, 0), (0, 0, 1), (1, 1, 0)):
        a_cells[0, (3 + d[0]) | (3 + d[1]) << 3 | (3 + d[2]) << 6] = STATIC
    res, sc = both(hdr, cells, (hdr, a_cells), radius=(1, 1, 1))
    k = lambda d: ((d[2] + 1) * 3 + d[1] + 1) * 3 + d[0] + 1  # noqa: E731
    assert sorted(np.nonzero(sc["n_oo"])[0].tolist()) == sorted([k((-1, 0, 0)), k((0, 0, 1)), k((1, 1, 0))])
    assert res["best"] == k((-1, 0, 0)) < k((0, 0, 1)) and res["best_score"] == 5
    assert res["runner_up"] == 5                          # (1, 1, 0) lies two cells from (-1, 0, 0)
    res, _ = both(hdr, cells, (hdr, a_cells), radius=(1, 1, 1), weights=(-1, 0, 0, 0, 0))
    assert res["best"] == 13 and res["best_score"] == 0   # every other candidate scores 0 too: the centre is nearest


def test_the_planted_offset_is_the_strict_unique_maximum():
    arch = mr.blob_scene()
    assert 300 <= (wr.occ_of(arch[1]) >= 1).sum() <= 3000
    hdr, cells = mr.shifted_copy(arch[0], arch[1], mr.PLANTED)
    assert (wr.occ_of(cells) >= 1).sum() == (wr.occ_of(arch[1]) >= 1).sum()
    for offset, radius in (((0, 0, 0), (4, 4, 2)), ((2, -4, 3), (3, 3, 2)), (mr.PLANTED, (0, 0, 0))):
        res, sc = mr.dense(hdr, cells, arch[0], arch[1], offset=offset, radius=radius)
        s = mr.score_of(sc, binding.WORLD_MATCH_WEIGHTS)
        best = sc[res["best"]]
        assert res["best_offset"].tolist() == list(mr.PLANTED) and (s == s.max()).sum() == 1
        assert best["n_of"] == 0 and best["n_fo"] == 0 and best["n_oo"] == res["src_occupied"] == best["n_same"]
        assert best["n_ff"] == res["src_free"] and (res["runner_up"] < res["best_score"] or radius == (0, 0, 0))
    # ... and over the wide search world_align tiles: nothing within (12, 12, 4) comes near it
    wide = max(mr.score_of(mr.dense(hdr, cells, arch[0], arch[1], offset=(ox, oy, 0), radius=(8, 8, 4))[1], binding.WORLD_MATCH_WEIGHTS)[
        [k for k, o in enumerate(mr.candidates((ox, oy, 0), (8, 8, 4))[1].tolist()) if tuple(o) != mr.PLANTED]].max()
        for ox in (-4, 4) for oy in (-4, 4))
    assert wide < s.max()
    small = mr.naive(hdr, cells, mr.naive_archive(*arch), offset=(2, -2, 1), radius=(1, 0, 0))
    assert small[1].tobytes() == mr.dense(hdr, cells, arch[0], arch[1], offset=(2, -2, 1), radius=(1, 0, 0))[1].tobytes()
