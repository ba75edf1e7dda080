"""The restatement of the travel-cost field (tests/reach_ref.py) against independent statements of the same thing: a
whole-grid Bellman-Ford sweep to the fixed point, SciPy's Dijkstra where SciPy is there, the closed form on an empty
block, hand cases for the corner rule; the properties of every descended path; the record sizes."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import reach_ref as rr

NO = rr.NO_COST


def random_trav(n, seed, p_free=0.7):
    return np.random.default_rng(seed).random((n, n, n)) < p_free


def word(shape, x, y, z):
    return x + shape[2] * (y + shape[1] * z)


@pytest.mark.parametrize("face", [False, True])
@pytest.mark.parametrize("n,seed", [(16, 1), (16, 2), (32, 3)])
def test_dijkstra_is_the_fixed_point_of_the_sweeps(n, seed, face):
    trav = random_trav(n, seed)
    starts = np.random.default_rng(seed + 100).integers(0, n ** 3, 3)
    for max_cost in (0, 150):
        a = rr.dijkstra(trav, starts, face, max_cost)
        b = rr.bellman_ford(trav, starts, face, max_cost)
        assert np.array_equal(a, b), (max_cost, int((a != b).sum()))
        assert (a != NO).sum() > (10 if max_cost else 100)
    full, cut = rr.dijkstra(trav, starts, face, 0), rr.dijkstra(trav, starts, face, 150)
    assert np.array_equal(cut, np.where(full <= 150, full, NO))   # a truncated search is still exact
    assert ((full > 150) & (full != NO)).any()


@pytest.mark.parametrize("face", [False, True])
def test_dijkstra_against_scipy(face):
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    trav = random_trav(16, 7)
    allowed = rr.allowed_bits(trav, face).ravel()
    rows, cols, vals = [], [], []
    for n, off, w in rr._flat_moves(trav.shape, face):
        src = np.flatnonzero((allowed >> np.uint32(n)) & 1)
        rows.append(src), cols.append(src + off), vals.append(np.full(len(src), w))
    g = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(trav.size, trav.size))
    starts = rr.start_words(trav, [5, 1000, 4000, 2222])
    assert len(starts) >= 1
    d = csgraph.dijkstra(g, directed=True, indices=starts, min_only=True)
    want = np.where(np.isfinite(d), d, NO).astype(np.uint32).reshape(trav.shape)
    assert np.array_equal(rr.dijkstra(trav, starts, face), want)


def test_closed_form_on_an_empty_block():
    trav = np.ones((12, 9, 14), bool)
    s = (5, 3, 7)
    cost = rr.dijkstra(trav, [word(trav.shape, *s)])
    z, y, x = np.meshgrid(*(np.arange(n) for n in trav.shape), indexing="ij")
    d = np.sort(np.stack([np.abs(x - s[0]), np.abs(y - s[1]), np.abs(z - s[2])]), axis=0)   # c <= b <= a
    assert np.array_equal(cost, (17 * d[0] + 14 * (d[1] - d[0]) + 10 * (d[2] - d[1])).astype(np.uint32))
    face = rr.dijkstra(trav, [word(trav.shape, *s)], face_connected=True)
    assert np.array_equal(face, (10 * d.sum(axis=0)).astype(np.uint32))


def test_the_move_numbers_and_weights():
    assert rr.move_offset(0) == (-1, -1, -1) and rr.move_offset(14) == (1, 0, 0) and rr.move_offset(22) == (0, 0, 1)
    assert [rr.move_weight(n) for n in (0, 1, 4, 12)] == [17, 14, 10, 10]
    assert sorted(rr.move_weight(n) for n in rr.MOVES) == [10] * 6 + [14] * 12 + [17] * 8


def test_corner_rule_two_cells_that_share_an_edge():
    """# G    in the plane z = 1 of a 3 x 3 x 3 block the cells (0, 0) and (1, 1) are blocked: they share an edge, and the
       S #    diagonal from S = (0, 1) to G = (1, 0) between them is refused.  The way round goes through another layer."""
    trav = np.ones((3, 3, 3), bool)
    trav[1, 0, 0] = trav[1, 1, 1] = False
    shape = trav.shape
    s, g = word(shape, 0, 1, 1), word(shape, 1, 0, 1)
    al = rr.allowed_bits(trav)
    assert not (int(al.ravel()[s]) >> (1 * 9 + 0 * 3 + 2)) & 1    # (dx, dy, dz) = (+1, -1, 0)
    assert not (int(al.ravel()[s]) >> (0 * 9 + 0 * 3 + 2)) & 1    # (+1, -1, -1): its cube holds both blocked cells
    assert (int(al.ravel()[s]) >> (0 * 9 + 1 * 3 + 1)) & 1        # (0, 0, -1)
    f = rr.Field(trav, [s])
    assert f.cost.ravel()[g] == 10 + 14 + 10   # down a layer, the same diagonal there (both of its side cells are free), up again
    p = f.path(g)
    assert rr.check_path(f, p) is None and len(p) == 4
    # the same layer alone: the way round stays in the plane
    flat = trav[1:2].copy()
    assert rr.dijkstra(flat, [word(flat.shape, 0, 1, 0)]).ravel()[word(flat.shape, 1, 0, 0)] == 60
    # ... and the 2 x 2 square alone: no way round, the goal is unreachable
    sq = flat[:, :2, :2].copy()
    assert rr.dijkstra(sq, [word(sq.shape, 0, 1, 0)]).ravel()[word(sq.shape, 1, 0, 0)] == NO


def test_corner_rule_two_cells_that_share_a_corner():
    """a 3-D diagonal needs all the seven other cells of its cube: with two blocked cells that share one corner only, the
    diagonal of their cube is refused - and so is every edge move of the cube, each of whose squares holds one of the two"""
    trav = np.ones((2, 2, 2), bool)
    trav[0, 0, 1] = trav[1, 1, 0] = False   # (x, y, z) = (1, 0, 0) and (0, 1, 1)
    s, g = word(trav.shape, 0, 0, 0), word(trav.shape, 1, 1, 1)
    al = rr.allowed_bits(trav)
    assert not (int(al.ravel()[s]) >> 26) & 1 and not (int(al.ravel()[g]) >> 0) & 1
    f = rr.Field(trav, [s])
    assert f.cost.ravel()[g] == 30   # three face moves
    assert rr.check_path(f, f.path(g)) is None and len(f.path(g)) == 4
    # one blocked cell: the diagonal is still refused, an edge move and a face move remain
    one = np.ones((2, 2, 2), bool)
    one[0, 0, 1] = False
    f1 = rr.Field(one, [s])
    assert f1.cost.ravel()[g] == 24 and not (int(f1.allowed.ravel()[g]) >> 0) & 1


@pytest.mark.parametrize("face", [False, True])
def test_every_descended_path(face):
    trav = random_trav(16, 21, 0.6)
    f = rr.Field(trav, [word(trav.shape, 8, 8, 8), word(trav.shape, 2, 3, 4), 1 << 20, 77], face_connected=face)
    reached = np.flatnonzero(f.cost.ravel() != NO)
    assert len(reached) > 500
    for c in reached[:: max(1, len(reached) // 400)]:
        p = f.path(int(c))
        assert rr.check_path(f, p) is None, (c, rr.check_path(f, p))
    assert f.path(int(np.flatnonzero(~trav.ravel())[0])) == []
    q = f.query(0.25, cells=[int(reached[-1]), int(np.flatnonzero(~trav.ravel())[0]), trav.size + 5, int(rr.start_words(trav, [77, word(trav.shape, 8, 8, 8)])[0])])
    assert list(q["status"]) == [0, 2, 3, 0] and q["next"][3] == 13 and q["next"][1] == 255 and q["metres"][2] == -1.0
    assert q["cell"][2] == NO and q["metres"][0] == np.float32(q["cost"][0]) * (np.float32(0.25) * np.float32(0.1))


def test_record_sizes():
    class Info(C.Structure):
        _fields_ = [(k, C.c_uint32) for k in binding.REACH_INFO.names]

    class Result(C.Structure):
        _fields_ = [("cost", C.c_uint32), ("metres", C.c_float), ("cell", C.c_uint32), ("next", C.c_uint8), ("status", C.c_uint8),
                    ("pad", C.c_uint16)]
    assert C.sizeof(Info) == 32 and binding.REACH_INFO.itemsize == 32
    assert C.sizeof(Result) == 16 and binding.REACH_RESULT.itemsize == 16
    assert [binding.REACH_RESULT.fields[k][1] for k in binding.REACH_RESULT.names] == [0, 4, 8, 12, 13, 14]
    assert [getattr(Result, k).offset for k in binding.REACH_RESULT.names] == [0, 4, 8, 12, 13, 14]
