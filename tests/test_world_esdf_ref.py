"""The two restatements of the world distance field (tests/world_esdf_ref.py) against each other on every case of
tests/world_esdf_cases.py - coords, d2, offset and info -, against what is known in closed form, and the three
discrimination checks: a model without the wrap mask of the x shifts is wrong on the x-wrap case, a model with a halo of
one brick at R = 16 is wrong on the far-reach cases, and a model that scans descending names the wrong obstacle on every
tie.  No GPU."""
import numpy as np
import pytest

from tests import world_esdf_cases as ec
from tests import world_esdf_ref as wer

CASES = ec.crafted()
MM = ec.MM
NONE = ec.NONE


def cell_of(model, c):
    """(d2, offset) of world cell c in a model's field"""
    b, w = ec.word_of(c)
    r = model.coords.astype(np.int64).tolist().index(list(b))
    return int(model.d2[r, w]), tuple(int(v) for v in model.offset[r, w])


def both(c, **more):
    kw = dict(c["kw"], **more)
    a = wer.BrickModel(c["hdr"], c["cells"], max_movable=MM, **kw)
    b = wer.CellModel(c["hdr"], c["cells"], max_movable=MM, **kw)
    diff = wer.difference(wer.answer(a), wer.answer(b))
    assert diff is None, diff
    # what holds of every field: an offset is as long as its d2 says, NONE has no offset, the counts are the field's
    off = a.offset.astype(np.int64)
    near = a.d2 != NONE
    assert ((off * off).sum(axis=2)[near] == a.d2[near]).all() and (off[~near] == 0).all() and (a.d2[near] <= kw["radius"] ** 2).all()
    assert a.info["n_near_cells"] == near.sum() and a.info["n_obstacle_cells"] == (a.d2 == 0).sum()
    return a


def lattice_ball(radius, inside):
    """how many offsets o with |o|^2 <= radius^2 satisfy inside(o)"""
    ax = range(-radius, radius + 1)
    return sum(1 for x in ax for y in ax for z in ax if x * x + y * y + z * z <= radius * radius and inside((x, y, z)))


def check_closed_forms(name, a):
    """what the issue states about a case; the GPU test asserts the same of the library"""
    c = CASES[name]
    R = c["kw"]["radius"]
    if name.startswith("ball"):
        skip, solid = "skip" in name, "solid" in name
        assert a.info["n_bricks"] == (7 if skip else 8)
        cells = a.coords.astype(np.int64)[:, None, :] * 8 + np.stack([np.arange(512) & 7, (np.arange(512) >> 3) & 7, np.arange(512) >> 6], 1)[None]
        d2 = (cells * cells).sum(axis=2)                          # the obstacle is world cell (0, 0, 0)
        if not solid:
            assert np.array_equal(a.d2, np.where(d2 <= R * R, d2, NONE).astype(np.uint16))
            assert np.array_equal(a.offset.astype(np.int64), np.where((d2 <= R * R)[..., None], -cells, 0))
            in_bricks = lambda o: all(-8 <= v <= 7 for v in o) and not (skip and all(v < 0 for v in o))  # noqa: E731
            assert a.info["n_near_cells"] == lattice_ball(R, in_bricks) and a.info["n_obstacle_cells"] == 1
        else:                                                     # the missing brick is solid: cells (-8 .. -1)^3
            to_brick = (np.maximum(cells + 1, 0) ** 2).sum(axis=2)   # the nearest cell of it is min(c, -1) per axis
            outside = np.minimum(cells + 9, 8 - cells).min(axis=2)   # ... and so is everything round the eight bricks
            want = np.minimum(np.minimum(d2, to_brick), outside * outside)
            assert np.array_equal(a.d2, np.where(want <= R * R, want, NONE).astype(np.uint16))
    elif name == "x wrap" or name.startswith("ties"):
        assert cell_of(a, c["probe"]) == c["want"]
    elif name.startswith("far") or name.startswith("absent between") or name == "box":
        for cell, want in c["probes"]:
            assert cell_of(a, cell)[0] == want, (cell, want)
        if "n_bricks" in c:
            assert a.info["n_bricks"] == c["n_bricks"]
        if name.startswith("far 16"):
            axis = "xyz".index(name[-1])
            lo, hi = [0, 0, 0], [0, 0, 0]
            lo[axis], hi[axis] = -16, 16
            assert cell_of(a, ec.along(axis, 0)) == (256, tuple(lo)) and cell_of(a, ec.along(axis, 7)) == (256, tuple(hi))
        if name == "far diagonal":
            assert cell_of(a, (0, 0, 3)) == (244, (-12, -10, 0))
    elif name.startswith("int16 edge"):
        assert a.info["n_bricks"] == 12
        if not c["kw"]["unknown_is_obstacle"]:
            assert (a.d2 == NONE).all() and a.info["n_near_cells"] == 0      # nothing beyond the edge exists
        else:                                                                 # every side of every brick is solid but none of its cells
            w = np.arange(512)
            side = np.minimum(np.stack([w & 7, (w >> 3) & 7, w >> 6], 1), 7 - np.stack([w & 7, (w >> 3) & 7, w >> 6], 1)).min(axis=1) + 1
            assert (a.d2 == np.where(side <= R, side * side, NONE)[None]).all() and a.info["n_obstacle_cells"] == 0
    elif name.startswith("pillars"):
        assert a.info["n_bricks"] == 17 and 0 < a.info["n_obstacle_cells"] < a.info["n_near_cells"] < 17 * 512
    else:
        raise AssertionError(name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_restatements_agree(name):
    check_closed_forms(name, both(CASES[name]))


def test_static_only_drops_the_moving_pillars():
    a, b = both(CASES["pillars static_only=False"]), both(CASES["pillars static_only=True"])
    assert a.info["n_obstacle_cells"] > b.info["n_obstacle_cells"] > 0 and a.info["n_near_cells"] > b.info["n_near_cells"]


RANDOM = ec.random_archive()


@pytest.mark.parametrize("kw", ec.random_variants(), ids=lambda kw: " ".join("%s=%s" % (k, v) for k, v in sorted(kw.items())))
def test_the_two_restatements_agree_on_the_random_archive(kw):
    a = both(dict(hdr=RANDOM[0], cells=RANDOM[1], kw=kw))
    check_random(a, kw)


def check_random(a, kw):
    """no build is trivially empty or full: NONE, 0 and values in between all occur"""
    assert (a.d2 == NONE).any() and (a.d2 == 0).any() and ((a.d2 > 0) & (a.d2 != NONE)).any()
    assert a.info["n_bricks"] == (18 if kw["box"] else 122)
    if kw["radius"] == 16:
        assert ((a.d2 > 64) & (a.d2 != NONE)).any() and (np.abs(a.offset.astype(np.int64)) > 8).any()   # across two bricks


def test_the_flags_change_the_random_field():
    seen = set()
    for u in (False, True):
        for s in (False, True):
            a = wer.BrickModel(RANDOM[0], RANDOM[1], radius=9, max_movable=MM, unknown_is_obstacle=u, static_only=s)
            seen.add(a.d2.tobytes())
    assert len(seen) == 4


def test_empty_fields():
    c = CASES["x wrap"]
    for box in (((100, 100, 100), (101, 101, 101)), ((0, 0, 0), (0, -1, 0))):
        a = both(c, box=box)
        assert a.info["n_bricks"] == 0 and a.d2.shape == (0, 512) and a.info["n_near_cells"] == 0
    a = both(dict(hdr=c["hdr"][:0], cells=c["cells"][:0], kw=c["kw"]))
    assert a.info["n_bricks"] == 0


def test_queries_of_the_model():
    c = CASES["far 16 x"]
    a = wer.BrickModel(c["hdr"], c["cells"], max_movable=MM, **c["kw"])
    size = np.float32(ec.CFG["voxel_size"])
    res = a.query([(0, 3, 3), (1, 3, 3), (-1, 3, 3), (0, 3, 40)], size)
    assert res["d2"].tolist() == [256, 0xFFFFFFFE, 225, 0xFFFFFFFF]
    assert res["nearest"].tolist() == [[-16, 3, 3], [1, 3, 3], [-16, 3, 3], [0, 3, 40]]
    assert res["distance"].tolist() == [np.float32(16) * size, np.sqrt(np.float32(257)) * size, np.float32(15) * size, -1.0]


# ---- the discrimination checks
def test_a_model_without_the_wrap_mask_is_wrong_on_the_x_wrap_case():
    c = CASES["x wrap"]
    wrong = wer.BrickModel(c["hdr"], c["cells"], max_movable=MM, wrap_mask=False, **c["kw"])
    assert cell_of(wrong, c["probe"])[0] == 1 and c["want"][0] == 50


@pytest.mark.parametrize("name", ["far 16 x", "far 16 y", "far 16 z", "far diagonal"])
def test_a_halo_of_one_brick_is_wrong_at_radius_16(name):
    c = CASES[name]
    wrong = wer.BrickModel(c["hdr"], c["cells"], max_movable=MM, halo=1, **c["kw"])
    right = wer.BrickModel(c["hdr"], c["cells"], max_movable=MM, **c["kw"])
    cell, want = c["probes"][0]
    assert cell_of(right, cell)[0] == want >= 244 and cell_of(wrong, cell)[0] == NONE


@pytest.mark.parametrize("kind", ["x", "y", "z", "three"])
def test_descending_scans_name_the_wrong_obstacle(kind):
    c = CASES["ties " + kind]
    wrong = wer.BrickModel(c["hdr"], c["cells"], max_movable=MM, descending=True, **c["kw"])
    d2, off = cell_of(wrong, c["probe"])
    assert d2 == c["want"][0] and off != c["want"][1]
    assert np.array_equal(wrong.d2, wer.CellModel(c["hdr"], c["cells"], max_movable=MM, **c["kw"]).d2)   # the distances agree
