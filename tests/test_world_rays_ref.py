"""The two restatements of world rays (tests/world_rays_ref.py) against each other and against the closed forms of
tests/world_rays_cases.py, no GPU: BrickWalk steps a DDA through a dict of bricks, DenseWalk sorts plane crossings over a
dense grid.  Every crafted segment and view and the random archive's 512 segments and 12 views, byte for byte.  Then the
discrimination checks: each of four plausible mistakes, switched on in BrickWalk, must change at least one crafted answer."""
import numpy as np
import pytest

from tests import world_rays_cases as rc
from tests import world_rays_ref as rr

SEGMENTS = rc.segment_cases()
VIEWS = rc.view_cases()


def models(arch, fault=None):
    return rr.BrickWalk(arch[0], arch[1], rc.SIZE, rc.MM, fault=fault), rr.DenseWalk(arch[0], arch[1], rc.SIZE, rc.MM)


def check_want(name, rec, want):
    """the fields a case states in closed form"""
    for k, v in want.items():
        got = rec[k]
        assert np.array_equal(np.asarray(got), np.asarray(v, np.asarray(got).dtype)), (name, k, got, v)


def segment_answer(model, c):
    return model.segments(c["a"][None], c["b"][None], **c["kw"])


def view_answer(model, c):
    return model.views(c["views"], c["dirs"], c["reach"], **c["kw"])


@pytest.mark.parametrize("name", sorted(SEGMENTS))
def test_crafted_segments(name):
    c = SEGMENTS[name]
    brick, dense = models(c["arch"])
    got = segment_answer(brick, c)
    assert got.tobytes() == segment_answer(dense, c).tobytes(), (name, got)
    check_want(name, got[0], c["want"])


@pytest.mark.parametrize("name", sorted(VIEWS))
def test_crafted_views(name):
    c = VIEWS[name]
    brick, dense = models(c["arch"])
    gain, rays = view_answer(brick, c)
    gain_d, rays_d = view_answer(dense, c)
    assert gain.tobytes() == gain_d.tobytes() and rays.tobytes() == rays_d.tobytes(), (name, gain, gain_d)
    check_want(name, gain[0], c["want"])
    assert (gain["pad"] == 0).all() and (gain["ray_cells"] == rays["cells"].sum(axis=1)).all()
    assert (rays["cells"] <= 3 * c["reach"] + 1).all()          # the window bounds a ray


def test_the_shared_cells_are_counted_once():
    g = view_answer(models(VIEWS["shared cells"]["arch"])[0], VIEWS["shared cells"])[0][0]
    assert g["ray_cells"] == 390 and g["n_free"] + g["n_unknown"] + g["n_occupied"] == 6


def test_rays_equal_segments_where_the_window_holds_them():
    """rays_out is what the segment query answers for (a, b) when the whole segment lies in the window"""
    from tests import views_ref as vr
    c = VIEWS["several views"]
    brick = models(c["arch"])[0]
    gain, rays = view_answer(brick, c)
    a, b, given = vr.rays_of(c["views"], c["dirs"])
    seg = brick.segments(a.reshape(-1, 3), b.reshape(-1, 3)).reshape(rays.shape)
    inside = given & (np.abs(np.floor(b) - np.floor(a)).max(axis=2) <= c["reach"])
    assert inside.sum() > 300 and rays[inside].tobytes() == seg[inside].tobytes()


def test_the_random_archive():
    arch = rc.random_archive()
    brick, dense = models(arch)
    a, b = rc.random_segments()
    seen = set()
    for kw in (dict(), dict(unknown_blocks=True), dict(ignore_movable=True), dict(unknown_blocks=True, ignore_movable=True)):
        got = brick.segments(a, b, **kw)
        assert got.tobytes() == dense.segments(a, b, **kw).tobytes(), kw
        seen.add(got.tobytes())
        hit = got["t"] >= 0
        # the mix: hits and misses, long walks, hits in archived bricks (under UNKNOWN_BLOCKS nearly every segment is blocked)
        assert hit.sum() > 50 and (got["stamp"][hit] > 0).any() and not (got["cells"] == -1).any()
        if not kw.get("unknown_blocks"):
            assert hit.sum() < len(a) - 50 and (got["unknown"][~hit] > 0).any() and (got["cells"] > 100).any()
    assert len(seen) == 4
    views, dirs = rc.random_views(), rc.PINHOLE
    for reach, kw in ((20, dict()), (6, dict(ignore_movable=True))):
        gain, rays = brick.views(views, dirs, reach, **kw)
        gain_d, rays_d = dense.views(views, dirs, reach, **kw)
        assert gain.tobytes() == gain_d.tobytes() and rays.tobytes() == rays_d.tobytes()
        # (a view may stand in an obstacle: its rays end where they start)
        assert (gain["n_unknown"] > 0).sum() >= 10 and (gain["n_free"] > 0).sum() >= 10 and (gain["n_occupied"] > 0).all()
        assert (gain["ray_cells"] > gain["n_unknown"].astype(np.int64) + gain["n_free"] + gain["n_occupied"]).all()


# ---- discrimination: a restatement with one mistake must disagree with the closed forms somewhere --------------------
def answers(fault):
    out = []
    for name in sorted(SEGMENTS):
        c = SEGMENTS[name]
        out.append(segment_answer(models(c["arch"], fault)[0], c).tobytes())
    for name in sorted(VIEWS):
        c = VIEWS[name]
        out.append(b"".join(a.tobytes() for a in view_answer(models(c["arch"], fault)[0], c)))
    return out


RIGHT = None


@pytest.mark.parametrize("fault,where", [("y_before_x", "diagonal, wall after the x step"), ("absent_is_free", "across an absent brick"),
                                         ("ray_sum", "shared cells"), ("truncate", "starts below zero")])
def test_a_mistake_changes_a_crafted_answer(fault, where):
    global RIGHT
    RIGHT = RIGHT or answers(None)
    wrong = answers(fault)
    names = sorted(SEGMENTS) + sorted(VIEWS)
    changed = [n for n, r, w in zip(names, RIGHT, wrong) if r != w]
    assert where in changed, (fault, changed)
