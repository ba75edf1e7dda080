"""tests/world_ref.py against itself: the brick model (a pool of 8 x 8 x 8 bricks behind a capacity) must say what the
naive model (a dict from world cell to word) says - on random blocks, after shifts of 1, 3, 7, 8, 9 and N / 4 cells of both
signs on every axis, at negative world coordinates, under every flag combination; merging a snapshot twice changes
nothing; the capacity rule drops exactly the highest-ranked new bricks.  No GPU."""
import numpy as np
import pytest

from tests import world_ref as wr

MAX_MOVABLE = 100
WORDS = np.array([wr.UNKNOWN, wr.UNKNOWN, 0, 0, 0, 1 << 24 | 7 << 16 | 3, 1 << 24 | 8 << 16 | 65528, 2 << 24 | 7 << 16 | 5, 2 << 24 | 9 << 16 | 60000],
                 np.uint32)
SHAPES = [(4, 4, 4), (4, 32, 16), (16, 8, 4)]     # (NX, NY, NZ): axes below a brick, a brick, several


def block(rng, N):
    return rng.choice(WORDS, size=tuple(N[::-1]))


def agree(A, nv, voxel_size=0.25):
    """the brick model's getters and lookups against the naive model"""
    hdr, cells = A.bricks()
    coords = [(int(h["bx"]), int(h["by"]), int(h["bz"])) for h in hdr]
    assert coords == nv.bricks()
    assert coords == sorted(coords, key=lambda b: (b[2], b[1], b[0]))
    occ = wr.occ_of(cells)
    assert np.array_equal(hdr["n_occupied"], (occ >= 1).sum(axis=1)) and np.array_equal(hdr["n_free"], (occ == 0).sum(axis=1))
    for k, b in enumerate(coords):                         # every word of every brick, by its cell word
        for w in range(0, 512, 7):
            g = (b[0] * 8 + (w & 7), b[1] * 8 + ((w >> 3) & 7), b[2] * 8 + (w >> 6))
            assert cells[k, w] == nv.word(g), (b, w)
    pts = A.occupied(voxel_size)
    want = nv.occupied()
    assert len(pts) == len(want) == int(A.info()["n_occupied"])
    size = np.float32(voxel_size)
    for p, g in zip(pts[::5], want[::5]):
        assert (p["x"], p["y"], p["z"]) == tuple(np.float32(v) * size for v in g)
        w = nv.word(g)
        assert (int(p["track"]), int(p["label"]), int(p["occ"])) == (w & 0xFFFF, (w >> 16) & 0xFF, w >> 24)
    if coords:
        info = A.info()
        lo = info["bmin"].astype(np.int64) * 8 - 3
        size3 = (info["bmax"].astype(np.int64) - info["bmin"] + 1) * 8 + 6
        reg = A.region(lo, size3)
        assert reg.shape == tuple(size3[::-1])
        idx = np.argwhere(np.ones(reg.shape, bool))[::11]
        assert all(reg[k, j, i] == nv.word((i + lo[0], j + lo[1], k + lo[2])) for k, j, i in idx.tolist())
        centres = ((idx[:, ::-1] + lo).astype(np.float32) + np.float32(0.5)) * size
        q = A.query_points(centres, voxel_size)
        assert np.array_equal(q["occ"], wr.occ_of(reg[tuple(idx.T)])) and np.array_equal(q["track"], reg[tuple(idx.T)] & 0xFFFF)
        assert ((q["stamp"] > 0) == np.array([(i + lo[0] >> 3, j + lo[1] >> 3, k + lo[2] >> 3) in set(coords) for k, j, i in idx.tolist()])).all()


@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("flags", wr.ALL_FLAGS)
def test_random_blocks_shifted_on_every_axis(N, flags):
    N = np.array(N)
    rng = np.random.default_rng(sum(N) + flags)
    A, nv = wr.Archive(1 << 14), wr.Naive()
    steps = np.array([-7, 2, -300])                          # negative world coordinates on two axes from the start
    gts = 1
    for a in range(3):
        for k in sorted({1, 3, 7, 8, 9, int(N[a]) // 4}):
            for d in (k, -k, -k, k):
                steps[a] += d
                snap = block(rng, N)
                wr.merge(A, snap, steps, gts, MAX_MOVABLE, flags)
                nv.merge(snap, steps, MAX_MOVABLE, flags)
                gts += 1
        agree(A, nv)
    info = A.info()
    assert info["n_updates"] == gts - 1 and info["stamp"] == gts - 1 and info["flags"] == flags and (info["bmin"] < 0).any()
    if flags & wr.STATIC_ONLY:
        assert not any(1 <= (w & 0xFFFF) <= MAX_MOVABLE and 1 <= (w >> 24) < 128 for w in nv.cell.values())
    if flags & wr.OBSERVED_ONLY:
        assert not any((w >> 24) == 2 for w in nv.cell.values())


def test_the_brick_view_is_the_block():
    rng = np.random.default_rng(1)
    for N, steps in (((4, 4, 4), (2, 3, 9)), ((16, 8, 4), (-5, 100, -1)), ((8, 8, 8), (4, 4, 4))):
        snap = block(rng, np.array(N))
        b0, nb, words = wr.brick_view(snap, steps)
        g0 = wr.block_origin(snap, steps)
        assert len(words) == nb.prod() and (nb <= (np.array(N) + 7) // 8 + 1).all()
        seen = 0
        for c in range(len(words)):
            t, kx = divmod(c, int(nb[0]))
            kz, ky = divmod(t, int(nb[1]))
            for w in range(512):
                i = np.array([(b0[0] + kx) * 8 + (w & 7), (b0[1] + ky) * 8 + ((w >> 3) & 7), (b0[2] + kz) * 8 + (w >> 6)]) - g0
                inside = ((i >= 0) & (i < N)).all()
                assert words[c, w] == (snap[i[2], i[1], i[0]] if inside else wr.UNKNOWN)
                seen += int(inside)
        assert seen == snap.size
    assert ((np.array([8, 8, 8]) + 7) // 8 + 1 == 2).all() and wr.brick_view(block(rng, np.array([8, 8, 8])), (4, 4, 4))[1].tolist() == [1, 1, 1]


def test_merging_a_snapshot_twice_changes_nothing():
    rng = np.random.default_rng(2)
    snap = block(rng, np.array([16, 8, 4]))
    A = wr.Archive(4096)
    wr.merge(A, snap, (5, -9, 33), 4, MAX_MOVABLE, 0)
    hdr, cells = A.bricks()
    wr.merge(A, snap, (5, -9, 33), 4, MAX_MOVABLE, 0)
    hdr2, cells2 = A.bricks()
    assert hdr.tobytes() == hdr2.tobytes() and cells.tobytes() == cells2.tobytes() and A.created_last == 0 and A.n_updates == 2
    # an unknown block erases nothing, and only the stamps of bricks with a writing cell move
    wr.merge(A, np.full_like(snap, wr.UNKNOWN), (5, -9, 33), 9, MAX_MOVABLE, 0)
    hdr3, cells3 = A.bricks()
    assert hdr3.tobytes() == hdr.tobytes() and cells3.tobytes() == cells.tobytes() and A.stamp == 9


def test_the_capacity_rule_drops_the_highest_ranked_new_bricks():
    rng = np.random.default_rng(3)
    N = np.array([16, 16, 16])
    snap = block(rng, N)
    steps = (3, -2, 7)
    full = wr.Archive(4096)
    wr.merge(full, snap, steps, 1, MAX_MOVABLE, 0)
    order = [full.coord[s] for s in full.order()]
    assert full.coord == order and len(order) == 27           # created in brick order
    A = wr.Archive(10)
    wr.merge(A, snap, steps, 1, MAX_MOVABLE, 0)
    assert A.coord == order[:10] and A.created_last == 10
    _, _, words = wr.brick_view(snap, steps)
    n_wr = wr.writes(words, MAX_MOVABLE, 0).sum(axis=1)
    assert A.dropped_last == int(n_wr[10:].sum()) > 0 and A.dropped_total == A.dropped_last
    nv = wr.Naive()
    nv.merge(snap, steps, MAX_MOVABLE, 0, skip_bricks=order[10:])
    agree(A, nv)
    # the bricks that are in keep taking writes, the others stay out and are counted again
    snap2 = block(rng, N)
    wr.merge(A, snap2, steps, 2, MAX_MOVABLE, 0)
    nv.merge(snap2, steps, MAX_MOVABLE, 0, skip_bricks=order[10:])
    agree(A, nv)
    assert A.created_last == 0 and A.dropped_total > A.dropped_last > 0 and len(A.coord) == 10
    # a block elsewhere whose bricks rank below and above the archived ones: the lowest-ranked new ones would get room
    B = wr.Archive(12)
    wr.merge(B, snap, steps, 1, MAX_MOVABLE, 0)
    assert B.coord == order[:12]
    wr.merge(B, snap, (3, -2, 7 - 64), 2, MAX_MOVABLE, 0)
    assert len(B.coord) == 12 and B.created_last == 0 and B.dropped_last == int(n_wr.sum())


def test_out_of_range_bricks_are_counted_and_never_created():
    rng = np.random.default_rng(4)
    snap = block(rng, np.array([4, 4, 4]))
    A = wr.Archive(64)
    wr.merge(A, snap, (262143, 0, 0), 1, MAX_MOVABLE, 0)     # x cells 262141 .. 262144: bricks 32767 and 32768
    assert A.out_of_range_last > 0 and all(c[0] == 32767 for c in A.coord) and A.dropped_last == 0
    q = A.query_points([[262144.5, 0.5, 0.5], [np.nan, 0, 0], [np.inf, 0, 0]], 1.0)
    assert q.tobytes() == np.array([(0, 0, -1, 0)] * 3, q.dtype).tobytes()
    assert wr.default_max_bricks([256, 256, 256]) == 131072 and wr.default_max_bricks([4, 4, 4]) == 4096
