"""tests/world_io_ref.py against itself: the brick model of import and retain must say what the naive model (world cell
plus offset, cell by cell) says - over random source sets, under all eight offset residues per axis, at negative
coordinates, with FILL, with duplicated sources, under the capacity rule and after retains.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import world_io_ref as io
from tests import world_ref as wr
from tests.test_world_ref import MAX_MOVABLE, WORDS

FLAG_SETS = [(0, False), (wr.STATIC_ONLY, False), (wr.OBSERVED_ONLY, True), (wr.STATIC_ONLY | wr.OBSERVED_ONLY, False), (0, True)]


def random_source(rng, n, lo=-3, hi=3, dup=0, p_unknown=None):
    """n distinct random bricks around the origin (negative coordinates included), `dup` of them repeated with other
    words and stamps further down the array, shuffled or not by the caller"""
    box = np.array(list(itertools.product(range(lo, hi), repeat=3)))
    coord = box[rng.choice(len(box), n, replace=False)]
    coord = np.concatenate([coord, coord[rng.choice(n, dup, replace=False)]]) if dup else coord
    hdr = io.make_headers(coord, 1, 1)
    hdr["first_stamp"] = rng.integers(1, 50, len(hdr))
    hdr["last_stamp"] = hdr["first_stamp"] + rng.integers(0, 50, len(hdr))
    return hdr, rng.choice(WORDS, size=(len(hdr), 512), p=p_unknown)


def agree(A, nv, tag=""):
    """headers (coordinates, counts, stamps) and every word of the brick model against the naive one"""
    hdr, cells = A.bricks()
    got = io.coords(hdr)
    assert got == nv.bricks() == sorted(got, key=lambda b: (b[2], b[1], b[0])), tag
    assert sorted(nv.stamps) == sorted(got), tag
    for k, b in enumerate(got):
        assert [int(hdr["first_stamp"][k]), int(hdr["last_stamp"][k])] == nv.stamps[b], (tag, b)
        g = np.array(b) * 8 + io._C
        want = np.array([nv.word(c) for c in g.tolist()], np.uint32)
        assert np.array_equal(cells[k], want), (tag, b)
    occ = wr.occ_of(cells) if len(hdr) else np.zeros((0, 512), np.int8)
    assert np.array_equal(hdr["n_occupied"], (occ >= 1).sum(axis=1)) and np.array_equal(hdr["n_free"], (occ == 0).sum(axis=1))
    assert len(nv.occupied()) == int(A.info()["n_occupied"])


def both(A, nv, hdr, cells, offset, flags=0, fill=False):
    """the import on both models; the naive one is told which bricks the capacity rule left out"""
    before = set(A.coord)
    io.import_bricks(A, hdr, cells, offset, MAX_MOVABLE, flags, fill)
    ghost = io.Naive()
    ghost.cell, ghost.stamps = dict(nv.cell), {b: list(s) for b, s in nv.stamps.items()}
    ghost.import_cells(hdr, cells, offset, MAX_MOVABLE, flags, fill)
    left_out = [b for b in ghost.bricks() if b not in set(A.coord)]
    assert not (set(left_out) & before)
    nv.import_cells(hdr, cells, offset, MAX_MOVABLE, flags, fill, skip_bricks=left_out)
    return left_out


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_every_offset_residue_on_every_axis(axis):
    rng = np.random.default_rng(10 + axis)
    for res in range(8):
        off = [8 * int(rng.integers(-3, 3)) + (res if a == axis else int(rng.integers(0, 8))) for a in range(3)]
        if res % 2:
            off = [-v for v in off]
        A, nv = io.Archive(4096), io.Naive()
        hdr, cells = random_source(rng, 12, dup=2)
        both(A, nv, hdr, cells, off)
        agree(A, nv, ("first", off))
        assert A.created_last == len(A.coord) > 0 and A.info()["n_updates"] == 0 and A.info()["n_bricks"] == len(A.coord)
        for flags, fill in FLAG_SETS:                      # ... and onto what is there, every flag set, with and without FILL
            hdr2, cells2 = random_source(rng, 10)
            held = {g: w for g, w in nv.cell.items()}
            both(A, nv, hdr2, cells2, [o + int(rng.integers(-9, 9)) for o in off], flags, fill)
            agree(A, nv, (off, flags, fill))
            if fill:
                assert all(nv.cell[g] == w for g, w in held.items())


def test_an_offset_of_whole_bricks_moves_the_bricks():
    rng = np.random.default_rng(1)
    hdr, cells = random_source(rng, 20, p_unknown=None)
    A = io.Archive(4096)
    io.import_bricks(A, hdr, cells, (8, -16, 24), MAX_MOVABLE)
    got_hdr, got_cells = A.bricks()
    known = (wr.occ_of(cells) >= 0).any(axis=1)
    want = sorted((c[0] + 1, c[1] - 2, c[2] + 3) for c, k in zip(io.coords(hdr), known) if k)
    assert sorted(io.coords(got_hdr)) == want and len(want) == 20
    for c, row in zip(io.coords(got_hdr), got_cells):
        i = io.coords(hdr).index((c[0] - 1, c[1] + 2, c[2] - 3))
        assert np.array_equal(row, cells[i]) and A.first_stamp[A.slot[c]] == hdr["first_stamp"][i] and A.last_stamp[A.slot[c]] == hdr["last_stamp"][i]


def test_the_lowest_index_of_duplicated_sources_wins_entirely():
    rng = np.random.default_rng(2)
    hdr, cells = random_source(rng, 6, dup=3)
    cells[6:] = rng.choice(WORDS[2:], size=(3, 512))        # the later copies know every cell: none of it may arrive
    hdr["last_stamp"][6:] = 1000
    for off in ((0, 0, 0), (3, -5, 9)):
        A, B = io.Archive(64), io.Archive(64)
        io.import_bricks(A, hdr, cells, off, MAX_MOVABLE)
        io.import_bricks(B, hdr[:6], cells[:6], off, MAX_MOVABLE)
        assert A.bricks()[0].tobytes() == B.bricks()[0].tobytes() and A.bricks()[1].tobytes() == B.bricks()[1].tobytes()
        assert max(A.last_stamp) < 1000
        # the order of the array matters in no other way
        p = rng.permutation(6)
        C_ = io.Archive(64)
        io.import_bricks(C_, hdr[:6][p], cells[:6][p], off, MAX_MOVABLE)
        assert C_.bricks()[0].tobytes() == B.bricks()[0].tobytes() and C_.bricks()[1].tobytes() == B.bricks()[1].tobytes()


def test_the_capacity_rule_ranks_the_new_destinations_in_brick_order():
    rng = np.random.default_rng(3)
    for off in ((0, 0, 0), (1, 2, 3)):
        hdr, cells = random_source(rng, 12, lo=-2, hi=2)
        full = io.Archive(4096)
        io.import_bricks(full, hdr, cells, off, MAX_MOVABLE)
        order = [full.coord[s] for s in full.order()]
        assert full.coord == order                           # created in brick order
        A, nv = io.Archive(8), io.Naive()
        held_hdr, held_cells = random_source(rng, 3, lo=5, hi=7)
        both(A, nv, held_hdr, held_cells, (0, 0, 0))
        assert len(A.coord) == 3
        left_out = both(A, nv, hdr, cells, off)
        assert A.coord[3:] == order[:5] and A.created_last == 5 and left_out == order[5:]
        agree(A, nv, ("capacity", off))
        nw = {d: 0 for d in order}
        ghost = io.Naive()
        ghost.import_cells(hdr, cells, off, MAX_MOVABLE)
        for g in ghost.cell:
            nw[tuple(v >> 3 for v in g)] += 1
        assert A.dropped_last == A.dropped_total == sum(nw[d] for d in order[5:]) > 0
        p = rng.permutation(len(hdr))                        # a shuffled source gives the same bytes
        B = io.Archive(8)
        io.import_bricks(B, held_hdr, held_cells, (0, 0, 0), MAX_MOVABLE)
        io.import_bricks(B, hdr[p], cells[p], off, MAX_MOVABLE)
        assert B.bricks()[0].tobytes() == A.bricks()[0].tobytes() and B.bricks()[1].tobytes() == A.bricks()[1].tobytes() and B.coord == A.coord


def test_unknown_sources_and_destinations_out_of_range_create_nothing():
    A = io.Archive(16)
    hdr = io.make_headers([[0, 0, 0], [32767, 0, 0]], 3, 4)
    cells = np.full((2, 512), wr.UNKNOWN, np.uint32)
    io.import_bricks(A, hdr, cells, (1, 2, 3), MAX_MOVABLE)
    assert not A.coord and A.created_last == 0 and A.out_of_range_last == 0 and A.info()["max_bricks"] == 16
    cells[1] = 0
    io.import_bricks(A, hdr, cells, (8, 0, 0), MAX_MOVABLE)
    assert not A.coord and A.out_of_range_last == 1 and A.dropped_last == 0
    io.import_bricks(A, hdr, cells, (1, 0, 0), MAX_MOVABLE)   # cells 1 .. 7 stay in brick 32767, cell 0 of the next is out of range
    assert A.coord == [(32767, 0, 0)] and A.out_of_range_last == 1 and (wr.occ_of(A.cells[0]) == 0).sum() == 7 * 64
    nv = io.Naive()
    nv.import_cells(hdr, cells, (1, 0, 0), MAX_MOVABLE)
    agree(A, nv, "range")
    with pytest.raises(AssertionError):
        io.import_bricks(A, hdr, cells, ((1 << 19) + 1, 0, 0), MAX_MOVABLE)


def test_retain_by_box_and_stamp():
    rng = np.random.default_rng(5)
    for kw in (dict(bmin=(-1, -1, -1), bmax=(1, 1, 1)), dict(min_last_stamp=40), dict(bmin=(-3, 0, -3), bmax=(2, 2, 2), min_last_stamp=25),
               dict(bmin=(0, 0, 0), bmax=(3, -1, 3))):
        A, nv = io.Archive(64), io.Naive()
        hdr, cells = random_source(rng, 40)
        both(A, nv, hdr, cells, (2, 0, -5))
        before = {c: (A.cells[s].copy(), A.first_stamp[s], A.last_stamp[s]) for c, s in A.slot.items()}
        pool = list(A.coord)
        removed = io.retain(A, **kw)
        assert removed == nv.retain(**kw) and removed == len(before) - len(A.coord)
        agree(A, nv, kw)
        assert A.coord == [c for c in pool if c in A.slot]          # dense, in the previous relative order
        for c, s in A.slot.items():
            assert np.array_equal(A.cells[s], before[c][0]) and (A.first_stamp[s], A.last_stamp[s]) == before[c][1:]
        if "bmax" in kw and kw["bmax"][1] < kw["bmin"][1]:
            assert not A.coord and removed == len(before) and A.info()["max_bricks"] == 64
        else:
            assert 0 < removed < len(before), kw
        # the room that was made is there for the next import, under the same rule
        hdr2, cells2 = random_source(rng, 40)
        both(A, nv, hdr2, cells2, (0, 0, 0))
        agree(A, nv, ("after", kw))
        assert len(A.coord) <= 64


def test_rounds_of_import_and_retain_at_a_small_capacity():
    rng = np.random.default_rng(6)
    A, nv = io.Archive(24), io.Naive()
    full = False
    for k in range(20):
        hdr, cells = random_source(rng, int(rng.integers(1, 12)), dup=int(rng.integers(0, 2)))
        flags, fill = FLAG_SETS[k % len(FLAG_SETS)]
        both(A, nv, hdr, cells, rng.integers(-20, 20, 3), flags, fill)
        full |= A.dropped_last > 0
        if k % 3 == 2:
            lo = rng.integers(-4, 0, 3)
            hi, stamp = lo + rng.integers(2, 7, 3), int(rng.integers(0, 30))
            assert io.retain(A, lo, hi, stamp) == nv.retain(lo, hi, stamp)
        agree(A, nv, k)
    assert full
