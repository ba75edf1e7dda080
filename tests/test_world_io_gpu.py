"""sdm_world_import and sdm_world_retain (include/sdm.h) against tests/world_io_ref.py, bit for bit, through world_info,
world_bricks, world_occupied and a world_region around the bricks (test_world_gpu.compare).

The archive needs a map only as a handle: most cases use shape A of tests/shape_cases.py (4 cells per axis) and feed
synthetic bricks.  Round trips of a real archive (also through save_world / load_world); offsets checked without the
restatement; the smallest source sets at which the kernels can go wrong; merges, FILL and the flags; the capacity rule;
duplicates; the coordinate range; device mode; the interplay with sdm_world_update; retain; rounds of all three at a small
capacity; the argument checks."""
import ctypes as C
import itertools

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import shape_cases as sc
from tests import world_io_ref as io
from tests import world_ref as wr
from tests import test_world_gpu as twg

pytestmark = pytest.mark.gpu

PARAMS = synth.PARAMS["vkitti2"]
INV = 1
CFG = sc.config("A")
MM = CFG["max_movable_track"]
FREE, MOVING, STATIC, GUESS_MOVING, GUESS_STATIC = 0, 1 << 24 | 7 << 16 | 3, 1 << 24 | 8 << 16 | (MM + 1), 2 << 24 | 7 << 16 | MM, 2 << 24 | 9 << 16 | 65535
WORDS = np.array([wr.UNKNOWN, wr.UNKNOWN, FREE, FREE, FREE, MOVING, STATIC, GUESS_MOVING, GUESS_STATIC], np.uint32)
SCAN_TILE = 2048                                          # csrc/primitives.hip: what one block of the scan takes in a pass


def handle():
    return binding.SdmMap(CFG, PARAMS, synth.noise_table())


def source(rng, coord, known=True):
    """random words for bricks at `coord`, random stamps; known: every brick has at least one cell that writes"""
    coord = np.asarray(coord, np.int64).reshape(-1, 3)
    hdr = io.make_headers(coord)
    hdr["first_stamp"] = rng.integers(1, 100, len(hdr))
    hdr["last_stamp"] = hdr["first_stamp"] + rng.integers(0, 100, len(hdr))
    cells = rng.choice(WORDS, size=(len(hdr), 512))
    if known:
        cells[np.arange(len(hdr)), rng.integers(0, 512, len(hdr))] = STATIC
    return hdr, cells


def random_coords(rng, n, lo, hi):
    box = np.array(list(itertools.product(range(lo, hi), repeat=3)))
    return box[rng.choice(len(box), n, replace=False)]


def both(g, A, hdr, cells, offset=(0, 0, 0), flags=0, fill=False, max_bricks=0, **kw):
    g.world_import(hdr, cells, offset=offset, fill=fill, static_only=bool(flags & wr.STATIC_ONLY), observed_only=bool(flags & wr.OBSERVED_ONLY),
                   max_bricks=max_bricks, **kw)
    io.import_bricks(A, hdr, cells, offset, MM, flags, fill)


def check(g, A, tag, region=True, cfg=CFG):
    """test_world_gpu.compare; region False (many bricks): everything but the dense region around them"""
    if region:
        return twg.compare(g, A, cfg, tag)
    info, want = g.world_info(), A.info()
    assert info.tobytes() == want.tobytes(), (tag, info, want)
    hdr, cells = g.world_bricks()
    want_hdr, want_cells = A.bricks()
    assert hdr.tobytes() == want_hdr.tobytes() and np.array_equal(cells, want_cells), tag
    pts, n = g.world_occupied()
    assert n == int(info["n_occupied"]) and pts.tobytes() == A.occupied(cfg["voxel_size"]).tobytes(), tag
    return info


def probe(g, A, rng):
    """one random cell of every brick around the origin, through the hash table"""
    b = np.array(list(itertools.product(range(-6, 7), repeat=3)))
    xyz = ((b * 8 + rng.integers(0, 8, b.shape)).astype(np.float32) + np.float32(0.5)) * np.float32(CFG["voxel_size"])
    assert g.query_world(xyz).tobytes() == A.query_points(xyz, CFG["voxel_size"]).tobytes()


def state(g):
    hdr, cells = g.world_bricks()
    return [g.world_info().tobytes(), hdr.tobytes(), cells.tobytes(), g.world_occupied()[0].tobytes()]


# ---- round trips
@pytest.mark.parametrize("off,sign", [(0, -1), (1, 1), (7, -1)])
def test_a_round_trip_reproduces_every_byte(off, sign, tmp_path):
    cfg = sc.config("B")
    g = twg.crafted(cfg, twg.offset_steps(cfg, off, sign), seed=50 + off)
    g.world_update()
    info, (hdr, cells), (pts, n_pts) = g.world_info(), g.world_bricks(), g.world_occupied()
    assert len(hdr) > 8 and n_pts > 0
    path = str(tmp_path / "world.npz")
    g.save_world(path)
    for k in range(2):
        g.world_clear()
        if k == 0:
            g.world_import(hdr, cells)
        else:
            assert g.load_world(path) == len(hdr)
        hdr2, cells2 = g.world_bricks()
        assert hdr2.tobytes() == hdr.tobytes() and cells2.tobytes() == cells.tobytes()         # headers: stamps and counts included
        pts2, n2 = g.world_occupied()
        assert n2 == n_pts and pts2.tobytes() == pts.tobytes()
        info2 = g.world_info()
        for f in ("n_bricks", "max_bricks", "n_occupied", "n_free", "bmin", "bmax"):
            assert np.array_equal(info2[f], info[f]), f
        assert info2["created_last"] == len(hdr) and info2["n_updates"] == 0 and info2["flags"] == 0 and info2["stamp"] == 0
    other = handle()                                       # voxels of 1 m: not this file's
    with pytest.raises(ValueError, match="voxel_size"):
        other.load_world(path)
    other.close()
    g.close()


# ---- offsets, without the restatement
@pytest.mark.parametrize("offset", [(8, -16, 24), (1, 0, 0), (0, 3, 0), (0, 0, 7), (1, 2, 3), (-1, -9, -17), (7, 7, 7)])
def test_an_offset_moves_the_region(offset):
    rng = np.random.default_rng(sum(offset) + 40)
    hdr, cells = source(rng, random_coords(rng, 14, -2, 2))
    lo, size = np.array([-24, -24, -24]), np.array([48, 48, 48])
    g = handle()
    g.world_import(hdr, cells)
    want = g.world_region(lo, size)
    assert (wr.occ_of(want) >= 0).sum() == (wr.occ_of(cells) >= 0).sum()
    g.world_clear()
    g.world_import(hdr, cells, offset=offset)
    assert np.array_equal(g.world_region(lo + np.array(offset), size), want)
    info = g.world_info()
    assert info["n_occupied"] == (wr.occ_of(cells) >= 1).sum() and info["n_free"] == (wr.occ_of(cells) == 0).sum()
    g.close()


# ---- the smallest source sets at which the kernels can go wrong
def around_a_hole():
    return [c for c in itertools.product((-1, 0, 1), repeat=3) if c != (0, 0, 0)]


SETS = {
    "one brick": ([[3, -2, 5]], [(1, 2, 3)]),
    "two adjacent": ([[0, 0, 0], [1, 0, 0]], [(1, 2, 3), (5, 0, 0), (-3, -3, 0)]),
    "a hole in the middle": (around_a_hole(), [(1, 2, 3), (0, 0, 0), (-8, 4, 0)]),
    "straddling zero": (list(itertools.product((-1, 0), repeat=3)), [(-3, 5, -1), (0, 0, -7), (9, -9, 1)]),
}


@pytest.mark.parametrize("name", list(SETS))
def test_small_source_sets(name):
    coord, offsets = SETS[name]
    rng = np.random.default_rng(len(coord))
    g = handle()
    for offset in offsets:
        hdr, cells = source(rng, coord)
        g.world_clear()
        A = io.Archive(4096)
        both(g, A, hdr, cells, offset)
        info = check(g, A, (name, offset))
        assert info["created_last"] == info["n_bricks"] > 0 and info["n_updates"] == 0
        if name == "one brick":
            assert info["n_bricks"] == 8
        if name == "a hole in the middle" and offset == (0, 0, 0):
            assert info["n_bricks"] == 26 and g.query_world([[4.5, 4.5, 4.5]])[0]["occ"] == -1
    g.close()


def test_more_destinations_than_one_block_of_the_scan_takes():
    rng = np.random.default_rng(7)
    coord = np.array(list(itertools.product(range(-6, 6), repeat=3)))         # 1728 sources, 13^3 = 2197 destinations of 13824 pairs
    hdr, cells = source(rng, coord)
    g = handle()
    A = io.Archive(4096)
    both(g, A, hdr[rng.permutation(len(hdr))], cells, (1, 2, 3))
    info = check(g, A, "13^3", region=False)
    assert info["n_bricks"] == 13 ** 3 > SCAN_TILE
    lo, size = np.array([-60, -10, 30]), np.array([40, 24, 24])
    assert np.array_equal(g.world_region(lo, size), A.region(lo, size))
    g.close()


def test_two_thousand_random_bricks_into_a_capacity_that_ends_exactly_full():
    rng = np.random.default_rng(8)
    hdr, cells = source(rng, random_coords(rng, 2000, -8, 8))
    g = handle()
    A = io.Archive(2000)
    both(g, A, hdr, cells, max_bricks=2000)
    info = check(g, A, "full", region=False)
    assert info["n_bricks"] == info["max_bricks"] == info["created_last"] == 2000 and info["dropped_last"] == 0
    lo, size = np.array([-64, -64, -8]), np.array([128, 128, 16])
    assert np.array_equal(g.world_region(lo, size), A.region(lo, size))
    extra, extra_cells = source(rng, [[20, 20, 20], [-20, 0, 0]])               # no room: dropped, and what is there still merges
    both(g, A, np.concatenate([extra, hdr[:50]]), np.concatenate([extra_cells, cells[50:100]]))
    info = check(g, A, "full again", region=False)
    assert info["created_last"] == 0 and info["dropped_last"] == (wr.occ_of(extra_cells) >= 0).sum() == info["dropped_total"]
    g.close()


# ---- merging into an archive that holds something
def test_overwrite_and_fill():
    rng = np.random.default_rng(9)
    coord = random_coords(rng, 10, -1, 2)
    held, held_cells = source(rng, coord)
    held["first_stamp"], held["last_stamp"] = 50, 60
    inc, inc_cells = source(rng, np.concatenate([coord[:6], [[5, 5, 5]]]))
    inc["first_stamp"], inc["last_stamp"] = [40, 55, 40, 55, 40, 55, 7], [58, 58, 70, 70, 58, 70, 9]
    for fill in (False, True):
        g = handle()
        A = io.Archive(4096)
        both(g, A, held, held_cells)
        before_hdr, before_cells = g.world_bricks()
        both(g, A, inc, inc_cells, fill=fill)
        check(g, A, ("fill", fill))
        hdr, cells = g.world_bricks()
        at = {c: k for k, c in enumerate(io.coords(hdr))}
        was = {c: k for k, c in enumerate(io.coords(before_hdr))}
        for i, c in enumerate(io.coords(inc)[:6]):
            got, old, new = cells[at[c]], before_cells[was[c]], inc_cells[i]
            if fill:                                       # every known resident cell is unchanged, the unknown ones take what comes
                known = wr.occ_of(old) >= 0
                assert np.array_equal(got[known], old[known]) and np.array_equal(got[~known], new[~known])
            else:                                          # every known incoming cell reads back
                known = wr.occ_of(new) >= 0
                assert np.array_equal(got[known], new[known]) and np.array_equal(got[~known], old[~known])
            wrote = (wr.occ_of(new) >= 0) & ((wr.occ_of(old) < 0) if fill else True)
            assert wrote.any()                             # stamps follow min / max
            assert hdr[at[c]]["first_stamp"] == min(50, inc["first_stamp"][i]) and hdr[at[c]]["last_stamp"] == max(60, inc["last_stamp"][i])
        for c in io.coords(held)[6:]:                      # untouched bricks: every byte
            assert hdr[at[c]].tobytes() == before_hdr[was[c]].tobytes() and cells[at[c]].tobytes() == before_cells[was[c]].tobytes()
        assert (hdr[at[(5, 5, 5)]]["first_stamp"], hdr[at[(5, 5, 5)]]["last_stamp"]) == (7, 9)
        g.close()


def test_static_only_and_observed_only_apply_to_incoming_words():
    cells = np.full((1, 512), wr.UNKNOWN, np.uint32)
    cells[0, :5] = [FREE, MOVING, STATIC, GUESS_MOVING, GUESS_STATIC]
    hdr = io.make_headers([[1, 1, 1]], 4, 5)
    want = {0: [FREE, MOVING, STATIC, GUESS_MOVING, GUESS_STATIC], wr.STATIC_ONLY: [FREE, wr.UNKNOWN, STATIC, wr.UNKNOWN, GUESS_STATIC],
            wr.OBSERVED_ONLY: [FREE, MOVING, STATIC, wr.UNKNOWN, wr.UNKNOWN], wr.STATIC_ONLY | wr.OBSERVED_ONLY: [FREE, wr.UNKNOWN, STATIC, wr.UNKNOWN, wr.UNKNOWN]}
    g = handle()
    for flags in wr.ALL_FLAGS:
        g.world_clear()
        A = io.Archive(4096)
        both(g, A, hdr, cells, flags=flags)
        check(g, A, flags)
        assert g.world_bricks()[1][0, :6].tolist() == want[flags] + [wr.UNKNOWN]
        g.world_clear()                                    # ... the same words one cell further: the brick's first five cells move
        A = io.Archive(4096)
        both(g, A, hdr, cells, (1, 0, 0), flags=flags)
        check(g, A, (flags, "moved"))
        assert g.world_region([9, 8, 8], [5, 1, 1]).ravel().tolist() == want[flags]
    g.close()


# ---- capacity, duplicates, nothing to write, the range
def test_capacity_takes_the_lowest_in_brick_order():
    rng = np.random.default_rng(11)
    held, held_cells = source(rng, [[9, 9, 9], [9, 9, 8], [8, 9, 9]])
    hdr, cells = source(rng, random_coords(rng, 12, -2, 2))
    order = sorted(io.coords(hdr), key=lambda b: (b[2], b[1], b[0]))
    results = []
    for p in (np.arange(12), rng.permutation(12), rng.permutation(12)):
        g = handle()
        A = io.Archive(8)
        both(g, A, held, held_cells, max_bricks=8)
        both(g, A, hdr[p], cells[p])
        info = check(g, A, "capacity")
        assert info["n_bricks"] == info["max_bricks"] == 8 and info["created_last"] == 5
        got = io.coords(g.world_bricks()[0])
        assert sorted(got) == sorted(order[:5] + io.coords(held))
        left = [i for i, c in enumerate(io.coords(hdr)) if c in order[5:]]
        assert info["dropped_last"] == info["dropped_total"] == (wr.occ_of(cells[left]) >= 0).sum() > 0
        with pytest.raises(binding.SdmError, match="max_bricks"):
            g.world_import(hdr, cells, max_bricks=64)
        results.append(state(g))
        g.close()
    assert results[0] == results[1] == results[2]


def test_of_duplicated_sources_the_lowest_index_wins_entirely():
    rng = np.random.default_rng(12)
    hdr, cells = source(rng, [[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0], [2, 2, 2]])
    cells[2:5] = rng.choice(WORDS[2:], size=(3, 512))      # the copies know every cell: none of it may arrive
    hdr["last_stamp"][2:5] = 1000
    g = handle()
    for offset in ((0, 0, 0), (4, 4, 4)):
        g.world_clear()
        A = io.Archive(4096)
        both(g, A, hdr, cells, offset)
        check(g, A, ("duplicates", offset))
        first = state(g)
        g.world_clear()
        g.world_import(hdr[[0, 1, 5]], cells[[0, 1, 5]], offset=offset)
        assert state(g) == first and g.world_bricks()[0]["last_stamp"].max() < 1000
    g.close()


def test_an_all_unknown_brick_creates_nothing():
    g = handle()
    hdr = io.make_headers([[0, 0, 0], [4, 4, 4]], 2, 3)
    cells = np.full((2, 512), wr.UNKNOWN, np.uint32)
    A = io.Archive(64)
    both(g, A, hdr, cells, (1, 2, 3), max_bricks=64)
    info = check(g, A, "unknown")
    assert info["n_bricks"] == 0 and info["created_last"] == 0 and info["max_bricks"] == 64 and (info["bmax"] == -1).all()
    cells[1, 511] = FREE
    both(g, A, hdr, cells, (1, 2, 3))
    assert io.coords(g.world_bricks()[0]) == [(5, 5, 5)] and check(g, A, "one cell")["n_free"] == 1
    assert g.world_import(hdr[:0], cells[:0]) is None and state(g) == state(g)
    g.close()


def test_the_coordinate_range():
    g = handle()
    hdr = io.make_headers([[32767, 0, -32768], [0, 0, 0]], 1, 2)
    cells = np.full((2, 512), FREE, np.uint32)
    A = io.Archive(4096)
    both(g, A, hdr, cells, (8, 0, 0))
    info = check(g, A, "x + 1 brick", region=False)
    assert info["out_of_range_last"] == 1 and info["n_bricks"] == 1 and info["dropped_last"] == 0
    both(g, A, hdr, cells, (1, 0, -1))                     # of the four destinations of the brick at the corner one is inside the range
    info = check(g, A, "one cell over", region=False)
    assert info["out_of_range_last"] == 3 and (32767, 0, -32768) in io.coords(g.world_bricks()[0])
    lo, size = np.array([262130, -4, -262150]), np.array([20, 12, 12])           # (the bricks lie too far apart for one region around them)
    assert np.array_equal(g.world_region(lo, size), A.region(lo, size))
    for bad in ((1 << 19) + 1, -(1 << 19) - 1):
        with pytest.raises(binding.SdmError, match="cell_offset"):
            g.world_import(hdr, cells, offset=(0, bad, 0))
    before = g.world_bricks()
    both(g, A, hdr[1:], cells[1:], (1 << 19, -(1 << 19), 0))                     # the largest offset there is: beyond the range from anywhere
    info = check(g, A, "largest", region=False)
    assert info["out_of_range_last"] == 1 and info["created_last"] == 0 and g.world_bricks()[0].tobytes() == before[0].tobytes()
    far = io.make_headers([[-32768, 32767, 5]], 6, 7)
    both(g, A, far, cells[:1], (65535 * 8, -65535 * 8, 0))                       # ... and from one end of it to the other
    info = check(g, A, "end to end", region=False)
    assert info["created_last"] == 1 and (32767, -32768, 5) in io.coords(g.world_bricks()[0])
    assert g.world_region([262136, -262144, 40], [8, 8, 8]).tobytes() == cells[0].tobytes()
    g.close()


# ---- device mode
def test_device_mode_gives_what_host_mode_gives():
    # (the sources are buffers of the library's own runtime: torch sees no device in a process that runs next to it)
    rng = np.random.default_rng(13)
    hdr, cells = source(rng, random_coords(rng, 40, -3, 3))
    pad = 256

    def padded(g, a):
        raw = np.frombuffer(a.tobytes(), np.uint8)
        buf = np.full(len(raw) + 2 * pad, 0xA5, np.uint8)
        buf[pad:pad + len(raw)] = raw
        return g.device_put(buf), buf

    for offset, fill in (((0, 0, 0), False), ((1, 2, 3), False), ((-5, 0, 9), True)):
        want = handle()
        want.world_import(hdr[:20], cells[:20])
        want.world_import(hdr, cells, offset=offset, fill=fill)
        g = handle()
        g.world_import(hdr[:20], cells[:20])
        d_hdr, b_hdr = padded(g, hdr)
        d_cells, b_cells = padded(g, cells)
        g.world_import(d_hdr + pad, d_cells + pad, offset=offset, fill=fill, on_device=True, n=len(hdr))
        g.world_import(d_hdr + pad, d_cells + pad, offset=offset, fill=fill, on_device=True, n=len(hdr))   # (the work arrays are kept)
        g.synchronize()
        want.world_import(hdr, cells, offset=offset, fill=fill)
        assert state(g) == state(want) and g.world_info()["n_bricks"] > 20
        assert np.array_equal(g.device_download(d_hdr, len(b_hdr)), b_hdr) and np.array_equal(g.device_download(d_cells, len(b_cells)), b_cells)  # sources, canaries
        g.device_free(d_hdr)
        g.device_free(d_cells)
        g.close()
        want.close()


# ---- with sdm_world_update
def test_import_and_update_in_either_order_and_the_map_is_left_alone():
    cfg = CFG
    steps = [9, -3, 20]                                    # the block: world cells 7 .. 10, -5 .. -2, 18 .. 21
    rng = np.random.default_rng(14)
    hdr, cells = source(rng, [[0, -1, 2], [1, -1, 2], [1, 0, 2], [3, 3, 3]])
    runs = []
    for run in range(2):
        out = []
        for order in ("import first", "update first"):
            g = twg.crafted(cfg, steps, seed=21)
            voxels, dump = g.voxels().tobytes(), {k: v.tobytes() for k, v in g.dump_state().items()}
            A = io.Archive(4096)
            if order == "update first":
                twg.update(g, A, cfg, wr.STATIC_ONLY)
            both(g, A, hdr, cells, (2, 1, -3))
            info = check(g, A, (order, "import"))
            assert info["n_updates"] == (order == "update first") and info["flags"] == (wr.STATIC_ONLY if info["n_updates"] else 0)
            if order == "import first":
                twg.update(g, A, cfg, wr.STATIC_ONLY)
            both(g, A, hdr, cells, (0, 0, 0), fill=True)
            info = check(g, A, (order, "fill"))
            assert info["n_updates"] == 1 and info["stamp"] == g.ring_state()["global_time_stamp"]
            assert g.world_retain(bmin=(0, -1, 2), bmax=(1, 0, 2)) == io.retain(A, (0, -1, 2), (1, 0, 2)) > 0
            check(g, A, (order, "retain"))
            assert g.voxels().tobytes() == voxels and {k: v.tobytes() for k, v in g.dump_state().items()} == dump
            out.append(state(g))
            g.close()
        runs.append(out)
    assert runs[0] == runs[1]


# ---- retain
RETAINS = {"box": dict(bmin=(-2, -1, -2), bmax=(0, 2, 1)), "stamp": dict(min_last_stamp=120), "both": dict(bmin=(-1, -3, -3), bmax=(2, 2, 2), min_last_stamp=90),
           "empty box": dict(bmin=(0, 0, 0), bmax=(5, 5, -1))}


@pytest.mark.parametrize("name", list(RETAINS))
def test_retain(name):
    kw = RETAINS[name]
    rng = np.random.default_rng(15)
    hdr, cells = source(rng, random_coords(rng, 60, -3, 3))
    g = handle()
    A = io.Archive(256)
    both(g, A, hdr, cells, (3, 0, -2), max_bricks=256)
    before_hdr, before_cells = g.world_bricks()
    info0 = g.world_info()
    removed = g.world_retain(**kw)
    assert removed == io.retain(A, **kw)
    info = check(g, A, name)
    assert info["n_bricks"] == len(before_hdr) - removed and info["max_bricks"] == 256
    for f in ("created_last", "dropped_last", "out_of_range_last", "dropped_total", "n_updates"):
        assert info[f] == info0[f], f
    assert (removed == len(before_hdr)) if name == "empty box" else (0 < removed < len(before_hdr))
    hdr2, cells2 = g.world_bricks()
    kept = {c: k for k, c in enumerate(io.coords(hdr2))}
    gone = []
    for k, c in enumerate(io.coords(before_hdr)):
        if c in kept:                                      # kept bricks: every byte
            assert hdr2[kept[c]].tobytes() == before_hdr[k].tobytes() and cells2[kept[c]].tobytes() == before_cells[k].tobytes()
        else:
            gone.append(c)
    assert len(gone) == removed
    centres = (np.array(gone)[:, None, :] * 8 + io._C[None, ::37] + 0.5).reshape(-1, 3).astype(np.float32)
    assert g.query_world(centres).tobytes() == np.array([(0, 0, -1, 0)] * len(centres), binding.WORLD_CELL).tobytes()
    # the room that was made is there for the next import, under the rule with the new n_bricks
    more, more_cells = source(rng, random_coords(rng, 40, -4, 4))
    both(g, A, more, more_cells, (0, -1, 0))
    info = check(g, A, (name, "import after"))
    assert info["n_bricks"] <= 256 and info["created_last"] > 0
    assert g.world_retain() == 0 and state(g) == state(g)  # no bound at all: everything stays
    check(g, A, (name, "retain all"))
    g.close()


def test_an_update_after_a_retain_creates_again_what_the_block_sees():
    cfg = sc.config("B")
    g = twg.crafted(cfg, sc.crafted_steps(cfg), seed=5)
    A = io.Archive(12)
    twg.update(g, A, cfg, 0, max_bricks=12)
    info = check(g, A, "full", cfg=cfg)
    assert info["n_bricks"] == 12 and info["dropped_last"] > 0
    hdr, _ = g.world_bricks()
    rows = np.unique(hdr["by"])
    assert len(rows) > 1
    box = dict(bmin=(-32768, int(rows[1]), -32768), bmax=(32767, 32767, 32767))       # the bricks of the lowest y go
    assert g.world_retain(**box) == io.retain(A, **box) > 0
    left = check(g, A, "trimmed", cfg=cfg)["n_bricks"]
    assert 0 < left < 12
    twg.update(g, A, cfg, 0)
    info = check(g, A, "updated", cfg=cfg)
    assert info["n_bricks"] == 12 and info["created_last"] == 12 - left and info["n_updates"] == 2
    assert g.world_retain(bmin=(0, 0, 0), bmax=(-1, 0, 0)) == 12 == io.retain(A, (0, 0, 0), (-1, 0, 0))
    info = check(g, A, "emptied", cfg=cfg)
    assert info["n_bricks"] == 0 and info["max_bricks"] == 12 and info["n_updates"] == 2 and g.world_occupied()[1] == 0
    twg.update(g, A, cfg, 0)
    assert check(g, A, "again", cfg=cfg)["created_last"] == 12
    g.close()


def test_twenty_rounds_of_import_retain_and_update_at_a_small_capacity():
    cfg = CFG
    rng = np.random.default_rng(16)
    g = twg.crafted(cfg, [9, -3, 20], seed=22)            # the block's bricks: (0 .. 1, -1, 2)
    A = io.Archive(24)
    dropped = trimmed = 0
    for k in range(20):
        hdr, cells = source(rng, random_coords(rng, int(rng.integers(1, 14)), -2, 3), known=False)
        flags = wr.ALL_FLAGS[k % 4]
        both(g, A, hdr, cells, rng.integers(-12, 12, 3), flags, fill=bool(k % 5 == 1), max_bricks=24 if k == 0 else 0)
        dropped += int(A.dropped_last > 0)
        if k % 2:
            lo = rng.integers(-4, 1, 3)
            kw = dict(bmin=lo, bmax=lo + rng.integers(1, 6, 3), min_last_stamp=int(rng.integers(0, 60)))
            n = g.world_retain(**kw)
            assert n == io.retain(A, **kw)
            trimmed += n
        if k % 3 == 0:
            twg.update(g, A, cfg, flags)
        check(g, A, ("round", k), region=k % 5 == 4)
        probe(g, A, rng)
    assert dropped > 0 and trimmed > 0 and g.world_info()["n_updates"] == 7
    g.close()


# ---- the argument checks
def test_argument_errors():
    g = handle()
    L, h, vp = g.L, g.h, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o, r = np.zeros(1, binding.WORLD_IMPORT_OPTIONS), np.zeros(1, binding.WORLD_RETAIN_OPTIONS)
    hdr, cells = io.make_headers([[0, 0, 0]]), np.zeros((1, 512), np.uint32)
    got = C.c_int64(-7)
    assert L.sdm_world_retain(h, vp(r), C.byref(got)) == INV and b"sdm_world_update first" in L.sdm_last_error() and got.value == -7
    assert L.sdm_world_import(h, None, vp(hdr), vp(cells), 1) == INV
    assert L.sdm_world_import(h, vp(o), None, vp(cells), 1) == INV and L.sdm_world_import(h, vp(o), vp(hdr), None, 1) == INV
    assert L.sdm_world_import(h, vp(o), vp(hdr), vp(cells), -1) == INV and L.sdm_world_import(h, vp(o), vp(hdr), vp(cells), (1 << 21) + 1) == INV
    for flags in (0x04, 0x08, 0x40, 1 << 31):
        o["flags"] = flags
        assert L.sdm_world_import(h, vp(o), vp(hdr), vp(cells), 1) == INV and b"flag" in L.sdm_last_error()
    o["flags"] = 0
    for a in range(3):
        for bad in ((1 << 19) + 1, -(1 << 19) - 1, -(1 << 31)):
            o["cell_offset"][0] = 0
            o["cell_offset"][0, a] = bad
            assert L.sdm_world_import(h, vp(o), vp(hdr), vp(cells), 1) == INV
    o["cell_offset"][0] = 0
    for bad in (-1, (1 << 21) + 1):
        o["max_bricks"] = bad
        assert L.sdm_world_import(h, vp(o), vp(hdr), vp(cells), 1) == INV
    o["max_bricks"] = 0
    assert g.world_info()["max_bricks"] == 0              # nothing of the above made an archive
    assert L.sdm_world_import(h, vp(o), None, None, 0) == 0 and L.sdm_world_retain(h, vp(r), None) == INV      # n == 0 changes nothing
    assert L.sdm_world_import(h, vp(o), vp(hdr), vp(cells), 1) == 0
    assert L.sdm_world_retain(h, None, None) == INV
    r["flags"] = 1
    assert L.sdm_world_retain(h, vp(r), None) == INV and b"flag" in L.sdm_last_error()
    r["flags"] = 0
    assert L.sdm_world_retain(h, vp(r), None) == 0 and L.sdm_world_retain(h, vp(r), C.byref(got)) == 0 and got.value == 0
    assert g.world_info()["n_bricks"] == 1
    r["bmax"][0] = -1
    assert L.sdm_world_retain(h, vp(r), C.byref(got)) == 0 and got.value == 1 and g.world_info()["n_bricks"] == 0
    g.world_clear()
    assert L.sdm_world_retain(h, vp(r), None) == INV
    g.close()
    shard = binding.SdmMap(synth.CONFIGS["T0"], PARAMS, synth.noise_table(), shard_rank=0, shard_count=2)
    assert L.sdm_world_import(shard.h, vp(o), vp(hdr), vp(cells), 1) == INV and b"Z-slab shard" in L.sdm_last_error()
    assert L.sdm_world_retain(shard.h, vp(r), None) == INV and b"Z-slab shard" in L.sdm_last_error()
    shard.close()
