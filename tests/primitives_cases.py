"""Inputs, references and case tables for the device tests of the exclusive scan and the stable radix sort
(tests/test_primitives_gpu.py).  Plain numpy, importable without a GPU; tests/test_primitives_cases.py checks that the
generators have the properties the device tests rely on.  Generated arrays are cached and read-only: every test that
needs one gets the same bytes."""
import functools

import numpy as np

# The structure the sizes below are derived from (semantic_dsp_map_amd/csrc/primitives.hip: SCAN_TILE / RS_TILE,
# SCAN_ITEMS / RS_ITEMS, the 64-lane wavefront, RS_BITS, SCAN_ONEPASS_MAX_TILES).  The device tests use them to pick sizes
# on both sides of every edge and to tell which form of the scan a length takes; they name no kernel and count no launch.
TILE = 2048                # elements per workgroup of the scan and of the sort
ITEMS = 8                  # elements per thread
LANES = 64                 # threads per wavefront
RADIX_BITS = 9             # key bits per sort pass
ONEPASS_MAX_TILES = 512    # the scan is one launch up to this many tiles, two launches beyond

ONEPASS_MAX = ONEPASS_MAX_TILES * TILE      # 1048576: the longest one-launch scan
# the sort scans its digit histogram, 2^RADIX_BITS counters per tile of keys: that scan is one launch up to this many keys
SORT_ONEPASS_MAX = ONEPASS_MAX // (1 << RADIX_BITS) * TILE   # 4194304 = 2048 tiles of 2048 keys

SENTINEL = 0xDEADBEEF      # what output buffers hold before a call
BEYOND = 0xFFFFFFFF        # what inputs hold beyond a device-side count


def tiles(n):
    return (n + TILE - 1) // TILE


def one_launch(n):
    """does a scan of n elements take the one-launch form?"""
    return tiles(n) <= ONEPASS_MAX_TILES


def sort_passes(nbits):
    return (nbits + RADIX_BITS - 1) // RADIX_BITS


# ---- scan ------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [
    1, 2, ITEMS - 1, ITEMS, ITEMS + 1,                      # items per thread
    LANES - 1, LANES, LANES + 1,                            # wave edge
    255 * ITEMS, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1,   # last thread of a tile, tile edges
    100000,
    ONEPASS_MAX - 1, ONEPASS_MAX, ONEPASS_MAX + 1,          # the switch between the two forms
    (ONEPASS_MAX_TILES + 1) * TILE + 1,                     # 514 tiles: more than 256 predecessors per tile
    4194304 + 17,
]
SCAN_VALUES = ["small", "uniform32", "all_ones", "zero", "flags"]
# one scratch, zeroed once: for each form, and for the two in turn
SCAN_REUSE_ONE_LAUNCH = [TILE + 1, 1, ONEPASS_MAX, LANES + 1, ONEPASS_MAX, 2 * TILE + 1]
SCAN_REUSE_TWO_LAUNCH = [ONEPASS_MAX + 1, 4194304 + 17, ONEPASS_MAX + 1]
SCAN_REUSE_MIXED = [ONEPASS_MAX + 1, TILE + 1, 4194304 + 17, ONEPASS_MAX, 1, ONEPASS_MAX + 1]


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=32)
def scan_values(kind, n):
    """the scan inputs: "small" 0..8 (what the map's counts look like), "uniform32" over all of uint32 (the sum wraps
    about n / 2 times), "all_ones" 0xFFFFFFFF, "zero", "flags" 0/1 with ones only next to tile edges"""
    rng = np.random.default_rng([n, SCAN_VALUES.index(kind)])
    if kind == "small":
        a = rng.integers(0, 9, n, dtype=np.uint32)
    elif kind == "uniform32":
        a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    elif kind == "all_ones":
        a = np.full(n, 0xFFFFFFFF, np.uint32)
    elif kind == "zero":
        a = np.zeros(n, np.uint32)
    elif kind == "flags":
        a = np.zeros(n, np.uint32)
        a[0::TILE] = 1           # k * TILE
        a[TILE - 1::TILE] = 1    # k * TILE - 1
    else:
        raise KeyError(kind)
    return _frozen(a)


def scan_ref(a, count=None):
    """exclusive prefix sum of the first `count` elements, summed in uint64 and reduced mod 2^32"""
    a = np.asarray(a)[:count].astype(np.uint64)
    out = np.zeros(a.size, np.uint64)
    np.cumsum(a[:-1], out=out[1:])
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def tile_totals_ref(a, count, capacity):
    """what a two-launch scan leaves behind its scratch's fixed region (sdm_internal.h): the totals mod 2^32 of the tiles of TILE elements of
    the launch, counting only the first `count` elements"""
    padded = np.zeros(tiles(capacity) * TILE, np.uint64)
    m = min(count, capacity)
    padded[:m] = np.asarray(a)[:m]
    return (padded.reshape(-1, TILE).sum(1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- sort ------------------------------------------------------------------------------------------------------------
ALL_NBITS = list(range(1, 33))
PASS_SIZES = [TILE + 1, 2 * TILE + 1]          # every nbits runs at these: two and three tiles, the last one key long
VOXEL_NBITS = [7, 16, 19, 25, 28]              # x_n + y_n + z_n + 1 of the smallest, typical and largest maps
VOXEL_N = 9 * TILE + 1581                      # 20013
VOXEL_RUNS = [3, LANES, LANES + 1, 256, 2500]
SHAPE_NBITS = [7, 9, 16, 25, 28, 32]
SHAPE_N = 3 * TILE + 5
SHAPES = ["all_equal", "all_max", "sorted", "reversed", "top_digit", "middle_digit"]
SORT_SIZES = [1, LANES - 1, LANES, LANES + 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 300000, 777777, 1 << 20,
              SORT_ONEPASS_MAX, SORT_ONEPASS_MAX + 1]
SORT_SIZE_NBITS = [25, 28]
SORT_REUSE = [SORT_ONEPASS_MAX + 1, TILE + 1, SORT_ONEPASS_MAX + 1, 1, 300000]
SORT_REUSE_NBITS = 25

# ---- device-side count: (capacity, what runs there) -------------------------------------------------------------------
COUNT_CAP_SMALL = 3 * TILE + 5
COUNT_CAP_SCAN_TWO_LAUNCH = (ONEPASS_MAX_TILES + 1) * TILE + 3
COUNT_CAP_SORT_TWO_LAUNCH = SORT_ONEPASS_MAX + 1


def counts_for(capacity):
    return [0, 1, TILE - 1, TILE, TILE + 1, capacity - 1, capacity, capacity + 7]


@functools.lru_cache(maxsize=32)
def uniform_keys(n, nbits, seed=0):
    rng = np.random.default_rng([n, nbits, seed, 1])
    return _frozen(rng.integers(0, 1 << nbits, n, dtype=np.uint64).astype(np.uint32))


@functools.lru_cache(maxsize=32)
def random_vals(n, seed=0):
    rng = np.random.default_rng([n, seed, 2])
    return _frozen(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


@functools.lru_cache(maxsize=32)
def voxel_like_keys(n, nbits):
    """keys as the births' sort sees them: blocks of the sentinel 1 << (nbits - 1) (invalid candidates; about half of all
    keys) between runs of equal voxel keys of about VOXEL_RUNS lengths, in input order, so that runs start anywhere in a tile"""
    rng = np.random.default_rng([n, nbits, 3])
    sentinel = 1 << (nbits - 1)
    parts, have, i = [], 0, 0
    while have < n:
        run = VOXEL_RUNS[i % len(VOXEL_RUNS)] + int(rng.integers(0, 3)) * (i >= len(VOXEL_RUNS))
        gap = int(rng.integers(1, 2 * run + 2))
        parts.append(np.full(gap, sentinel, np.uint32))
        parts.append(np.full(run, int(rng.integers(0, sentinel)), np.uint32))
        have += gap + run
        i += 1
    return _frozen(np.concatenate(parts)[:n].copy())


def digit_shift(nbits, which):
    """shift of the top (which = -1) or of a middle digit of an nbits key; None if it has no such digit"""
    p = sort_passes(nbits)
    if which == -1:
        return RADIX_BITS * (p - 1)
    return RADIX_BITS * (p // 2) if p >= 3 else None


@functools.lru_cache(maxsize=32)
def shaped_keys(shape, n, nbits):
    """None where the shape does not exist at this width (a middle digit needs three passes)"""
    rng = np.random.default_rng([n, nbits, SHAPES.index(shape), 4])
    top = (1 << nbits) - 1
    if shape == "all_equal":
        k = np.full(n, int(rng.integers(0, top + 1)), np.uint64)
    elif shape == "all_max":
        k = np.full(n, top, np.uint64)
    elif shape in ("sorted", "reversed"):
        k = np.sort(rng.integers(0, top + 1, n, dtype=np.uint64))
        k = k if shape == "sorted" else k[::-1]
    else:
        shift = digit_shift(nbits, -1 if shape == "top_digit" else 0)
        if shift is None:
            return None
        width = min(RADIX_BITS, nbits - shift)
        rest = int(rng.integers(0, top + 1)) & ~(((1 << width) - 1) << shift)
        k = (rng.integers(0, 1 << width, n, dtype=np.uint64) << np.uint64(shift)) | np.uint64(rest)
    return _frozen(np.ascontiguousarray(k).astype(np.uint32))


def sort_ref(keys):
    """the order a stable sort gives"""
    return np.argsort(np.asarray(keys), kind="stable")


def digits(keys, nbits):
    """the 9-bit digits of the keys below nbits, lowest first"""
    k = np.asarray(keys).astype(np.uint64)
    return [(k >> np.uint64(s)) & np.uint64((1 << RADIX_BITS) - 1) for s in range(0, nbits, RADIX_BITS)]


def equal_runs(keys):
    """(start, length) of the maximal runs of equal consecutive keys"""
    k = np.asarray(keys)
    edges = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1], [True]]))
    return edges[:-1], np.diff(edges)
