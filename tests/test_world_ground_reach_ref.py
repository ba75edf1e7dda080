"""The two restatements of world ground reach (tests/world_ground_reach_ref.py) against each other on every case of
tests/world_ground_reach_cases.py, and both against the values worked out by hand there.  No GPU: the ground layer each
field stands on is tests/world_ground_ref.py's ColumnModel of the case's archive."""
import numpy as np
import pytest

from tests import world_ground_reach_cases as rc
from tests import world_ground_reach_ref as ref
from tests import world_ground_ref as wgr

CASES = rc.crafted()


def ground_of(c, **gkw):
    return wgr.ColumnModel(c["hdr"], c["cells"], max_movable=rc.MM, stamp=7, **(gkw or c["gkw"]))


def both(ground, starts, **kw):
    args = (ground.coords, ground.cells, ground.d2, ground.o, starts)
    dense, sparse = ref.DenseReach(*args, stamp=7, **kw), ref.SparseReach(*args, stamp=7, **kw)
    diff = ref.difference(ref.answer(dense), ref.answer(sparse))
    assert diff is None, diff
    assert dense.info.tobytes() == sparse.info.tobytes() and dense.info["stamp"] == 7 and dense.info["rounds"] == 0
    return dense, sparse


def same_answers(dense, sparse, goals, max_len):
    a, b = dense.query(goals, rc.SIZE), sparse.query(goals, rc.SIZE)
    assert a.tobytes() == b.tobytes()
    pa, pb = dense.paths(goals, max_len, rc.FILL), sparse.paths(goals, max_len, rc.FILL)
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    return a, pa


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_cases(name):
    c = CASES[name]
    dense, sparse = both(ground_of(c), c["starts"], **c["kw"])
    for m in (dense, sparse):
        c["expect"](m)
    goals = rc.sample_goals(sparse, c["up"], 6, seed=len(name))
    q, (rows, lens) = same_answers(dense, sparse, goals, 12)
    assert (q["status"][:2] == 3).all() and ((lens > 0) == (q["status"] == 0)).all()
    # a path ends at a start and costs what the field says
    long_rows, long_lens = sparse.paths(goals, 400, rc.FILL)
    for i in np.flatnonzero(q["status"] == 0).tolist():
        cells = long_rows[i, :long_lens[i]].tolist()
        assert rc.path_sum(sparse, c["up"], cells) == int(q["cost"][i])
        assert int(sparse.query([cells[-1]], rc.SIZE)["cost"][0]) == 0


def test_the_late_corner_needs_the_wake_up_across_the_corner():
    c = CASES["late corner"]
    _, sparse = both(ground_of(c), c["starts"], **c["kw"])
    woken = rc.emulate_rounds(sparse, corners=True)
    for col, v in woken.items():
        assert (rc.NO if v is None else v) == rc.cost_at(sparse, *col), col
    sides = rc.emulate_rounds(sparse, corners=False)
    d = rc.LATE_MARKS["d"]
    assert sides[d] == 150 and woken[d] == 144
    assert {k: sides[q] for k, q in rc.LATE_MARKS.items() if k != "d"} == dict(c=130, f1=140, f2=140)


def test_the_rounds_come_to_the_field_on_the_serpentine():
    c = CASES["serpentine face"]
    _, sparse = both(ground_of(c), c["starts"], **c["kw"])
    woken = rc.emulate_rounds(sparse, corners=True)
    assert all(v == rc.cost_at(sparse, *col) for col, v in woken.items())


def test_thresholds_beyond_the_radius_are_refused_by_the_models_too():
    c = CASES["clearance min_d2 R^2 + 1"]
    g = ground_of(c)
    with pytest.raises(AssertionError):
        ref.SparseReach(g.coords, g.cells, g.d2, g.o, c["starts"], min_d2=11)


@pytest.mark.parametrize("k", range(len(rc.RANDOM_GROUNDS)))
def test_the_random_archive(k):
    hdr, cells = rc.random_world()
    gkw = rc.RANDOM_GROUNDS[k]
    ground = ground_of(dict(hdr=hdr, cells=cells), **gkw)
    starts = rc.random_starts(ground)
    assert len(starts) == 32
    reached = 0
    for kw in rc.random_reaches():
        dense, sparse = both(ground, starts, **kw)
        reached = max(reached, int(sparse.info["n_reached"]) - int(sparse.info["n_starts_used"]))
        same_answers(dense, sparse, rc.sample_goals(sparse, gkw["up"], 5, seed=k), 9)
    assert reached >= 10                      # (beyond the starts themselves: the fields are not trivial)
