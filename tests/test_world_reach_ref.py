"""The two restatements of world reach (tests/world_reach_ref.py) against each other on every crafted case of
tests/world_reach_cases.py at full size - rows, info, query results and paths -, and against what is known in closed
form.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import world_reach_cases as wc
from tests import world_reach_ref as wrr

CASES = wc.crafted()
SIZE = np.float32(wc.CFG["voxel_size"])


def both(c, **more):
    kw = dict(c["kw"], **more)
    a = wrr.DenseField(c["hdr"], c["cells"], c["starts"], wc.MM, **kw)
    b = wrr.SparseField(c["hdr"], c["cells"], c["starts"], wc.MM, **kw)
    assert wrr.equal_fields(a, b) is None, wrr.equal_fields(a, b)
    goals = wc.sample_goals(a, 24, seed=7)
    qa, qb = a.query(SIZE, cells=goals), b.query(SIZE, cells=goals)
    assert wrr.equal_results(qa, qb) is None, wrr.equal_results(qa, qb)
    assert wrr.equal_results(a.query(SIZE, xyz=wrr.cell_centres(goals, SIZE)), b.query(SIZE, xyz=wrr.cell_centres(goals, SIZE))) is None
    for pa, pb, q in zip(a.paths(SIZE, cells=goals), b.paths(SIZE, cells=goals), qa):
        assert np.array_equal(pa, pb)
        assert len(pa) == 0 if q["status"] != 0 else (1 <= len(pa) <= q["cost"] // 10 + 1 and a.cost_of(tuple(pa[-1])) == 0)
    return a


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_restatements_agree(name):
    c = CASES[name]
    a = both(c)
    assert a.info["n_starts_used"] == len(np.unique(c["starts"], axis=0)) and a.info["n_reached"] > 0
    if "rooms_reached" in c:
        got = sum(a.cost_of(q) != wrr.NO_COST for q in itertools.product((-5, 4), repeat=3))
        assert got == c["rooms_reached"]
    if "marks" in c:
        assert [a.cost_of(q) for q in c["marks"]] == [550, 560, 560, 564]
    if "lonely" in c:
        assert a.info["n_reached"] == 512 * len(c["lonely"]) == a.info["n_traversable"] // 2
        assert all(a.cost_of(tuple(8 * v for v in b)) == wrr.NO_COST and a.trav_of(tuple(8 * v for v in b)) for b in c["lonely"])
    if name.startswith("shell"):   # nothing passes through the hole: the far side is reached round it
        assert a.cost_of((15, 4, 4)) > wc.closed_form((23, 0, 0), False) and not a.has_brick((4, 4, 4))
    if name.startswith("plate"):
        assert a.info["n_bricks"] == 2116 > 2048 and a.info["n_reached"] == a.info["n_traversable"] == 46 * 46 * 64
    if name == "corridor":
        assert a.info["n_reached"] == 96 and a.info["max_cost_reached"] == 950


@pytest.mark.parametrize("kw", wc.random_variants(), ids=lambda kw: " ".join("%s=%s" % (k, v) for k, v in sorted(kw.items())))
def test_the_two_restatements_agree_on_the_random_archive(kw):
    hdr, cells = wc.random_world()
    assert len(hdr) == 4 * 4 * 2 - 3
    a = both(dict(hdr=hdr, cells=cells, starts=np.array(wc.RANDOM_STARTS), kw=kw))
    if kw.get("max_cost"):   # the budget cuts the field, and what is left is the untruncated field's
        full = wrr.DenseField(hdr, cells, wc.RANDOM_STARTS, wc.MM, **dict(kw, max_cost=0))
        assert 0 < a.info["n_reached"] < full.info["n_reached"] and a.info["max_cost_reached"] <= kw["max_cost"]
        assert np.array_equal(a.cost, np.where(full.cost <= kw["max_cost"], full.cost, wrr.NO_COST))
    if kw.get("box"):
        assert 0 < a.info["n_bricks"] < len(hdr)


@pytest.mark.parametrize("face", [False, True])
@pytest.mark.parametrize("at", [(0, 0, 0), (-1, -1, -1), (32767, -32768, 5)])
def test_one_free_brick_in_closed_form(at, face):
    c = wc.one_brick(at)
    for f in (wrr.DenseField, wrr.SparseField):
        a = f(c["hdr"], c["cells"], c["starts"], wc.MM, face_connected=face)
        want = np.array([wc.closed_form((w & 7, (w >> 3) & 7, w >> 6), face) for w in range(512)], np.uint32)
        assert np.array_equal(a.cost[0], want) and a.coords.tolist() == [list(at)]
        assert a.info["n_reached"] == 512 and a.info["max_cost_reached"] == (210 if face else 119)
        far = tuple(8 * v + 7 for v in at)
        assert a.step(far)[0] == (4 if face else 0) and len(a.path(far)) == (22 if face else 8)


@pytest.mark.parametrize("r,skip", [(1, False), (1, True), (2, False), (2, True)])
def test_inflation_is_the_chebyshev_ball(r, skip):
    """one obstacle cell in the corner of a brick: with inflate r exactly the (2 r + 1)^3 cells round it are lost, across
    faces, edges and the corner of the eight bricks that meet there - and none in a brick that is missing"""
    c = CASES["ball inflate=%d skip=%s" % (r, skip)]
    a = wrr.DenseField(c["hdr"], c["cells"], c["starts"], wc.MM, **c["kw"])
    assert a.info["n_traversable"] == 512 * len(c["hdr"]) - ((2 * r + 1) ** 3 - (r ** 3 if skip else 0))
    assert not a.trav_of((-r, -r, 0)) and a.trav_of((-r - 1, 0, 0)) and not a.trav_of((r, r, r))


def test_an_inflated_field_is_still_a_field():
    for name in CASES:
        if name.startswith("pillars"):
            c = CASES[name]
            a = wrr.DenseField(c["hdr"], c["cells"], c["starts"], wc.MM, **c["kw"])
            plain = wrr.DenseField(c["hdr"], c["cells"], c["starts"], wc.MM, **dict(c["kw"], inflate=0))
            assert 1000 < a.info["n_reached"] < plain.info["n_reached"] and a.info["n_starts_used"] == 2, (name, a.info)
