"""Device unit tests of the hand-written scan and radix sort (semantic_dsp_map_amd/csrc/primitives.hip).

The first two tests go through the one-call hooks.  The rest hold the two primitives to their contract in
csrc/sdm_internal.h through the sequence hooks (sdm_test_scan_seq / sdm_test_sort_pairs_seq): calls back to back on one
scratch buffer of exactly the promised size, zeroed once, with guard words behind it.  Inputs, references and case tables
come from tests/primitives_cases.py.  Every comparison is exact and covers every element."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import primitives_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 100000, 4194304 + 17])
def test_exclusive_scan(n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 9, n, dtype=np.uint32)
    got = binding.test_scan(a)
    want = np.concatenate([[0], np.cumsum(a[:-1], dtype=np.uint64)]).astype(np.uint32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,nbits", [(1, 8), (64, 8), (2048, 9), (2049, 16), (300000, 25), (1 << 20, 31), (777777, 32)])
def test_radix_sort_pairs_is_stable(n, nbits):
    rng = np.random.default_rng(n + nbits)
    # few distinct keys -> long equal-key runs, which is what exercises stability
    hi = min((1 << nbits) - 1, 5000 if n > 10000 else 7)
    keys = rng.integers(0, hi + 1, n, dtype=np.uint64).astype(np.uint32)
    if nbits == 32 or nbits == 31:
        keys = (keys.astype(np.uint64) * ((1 << nbits) // (hi + 1))).astype(np.uint32)
    vals = np.arange(n, dtype=np.uint32)
    ko, vo = binding.test_sort_pairs(keys, vals, nbits)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(ko, keys[order])
    assert np.array_equal(vo, vals[order])


# ---- the sequence hooks ----------------------------------------------------------------------------------------------
def same(got, want, what):
    """exact equality of two arrays, naming the first element that differs"""
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: %d of %d differ, first at %d (tile %d, place %d in it): got %#x, want %#x"
                             % (what, int((got != want).sum()), got.size, i, i // pc.TILE, i % pc.TILE, int(got[i]), int(want[i])))


def first_words(n):
    s = np.cumsum([0] + list(n))
    return s[:-1], s[1:]


def run_scans(capacity, arrays, count=None, in_place=False, count_on_device=False):
    """One sequence of scans, checked in full: slice i of the output holds the reference of its first min(count, capacity)
    elements and, beyond them, what the buffer held before the call (the sentinel; in place, the input).  The guard words
    behind the scratch are intact; every sequence leaves the scratch's fixed region zero, a two-launch scan its tiles'
    totals behind it."""
    capacity = list(capacity)
    count = capacity if count is None else list(count)
    a = np.concatenate(arrays)
    before = a if in_place else np.full(a.size, pc.SENTINEL, np.uint32)
    out, guard_ok, scratch = binding.test_scan_seq(capacity, a, before, count=count, in_place=in_place,
                                                   count_on_device=count_on_device, want_scratch=True)
    assert guard_ok, "the scan wrote behind scan_scratch_elems(%d) words of scratch" % max(capacity)
    for i, (lo, hi) in enumerate(zip(*first_words(capacity))):
        m = min(count[i], capacity[i])
        what = "scan %d of %d, capacity %d, count %d" % (i, len(capacity), capacity[i], count[i])
        same(out[lo:lo + m], pc.scan_ref(arrays[i], m), what)
        same(out[lo + m:hi], before[lo + m:hi], what + ", beyond the count")
    launched = [i for i, k in enumerate(count) if count_on_device or k]
    if launched:
        fixed = binding.test_scratch_elems(False, 1)
        assert not scratch[:fixed].any(), "the scans left %d words of the scratch's fixed region set" % np.count_nonzero(scratch[:fixed])
        i = launched[-1]
        n = capacity[i] if count_on_device else count[i]
        if not pc.one_launch(n):
            same(scratch[fixed:fixed + pc.tiles(n)], pc.tile_totals_ref(arrays[i], count[i], n), "tile totals left by the last scan")
    return out


def run_sorts(capacity, nbits, keys, vals, count=None, count_on_device=False):
    """One sequence of sorts, checked in full: the pair of buffers each call names holds the stably sorted first
    min(count, capacity) pairs and, beyond them, what it held before the call (first pair: the input; second pair: the
    sentinel).  The call names pair (passes & 1).  Guard words intact, the scratch's one-launch scan region zero."""
    capacity = list(capacity)
    count = capacity if count is None else list(count)
    nbits = [nbits] * len(capacity) if np.isscalar(nbits) else list(nbits)
    k, v = np.concatenate(keys), np.concatenate(vals)
    fill = np.full(k.size, pc.SENTINEL, np.uint32)
    ko, vo, which, guard_ok, scratch = binding.test_sort_pairs_seq(capacity, nbits, k, v, fill, fill, count=count,
                                                                   count_on_device=count_on_device, want_scratch=True)
    assert guard_ok, "the sort wrote behind sort_scratch_elems(%d) words of scratch" % max(capacity)
    for i, (lo, hi) in enumerate(zip(*first_words(capacity))):
        m = min(count[i], capacity[i])
        what = "sort %d of %d, capacity %d, count %d, %d bits" % (i, len(capacity), capacity[i], count[i], nbits[i])
        if m or count_on_device:
            assert which[i] == pc.sort_passes(nbits[i]) & 1, what
        order = pc.sort_ref(keys[i][:m])
        same(ko[lo:lo + m], keys[i][:m][order], what + ", keys")
        same(vo[lo:lo + m], vals[i][:m][order], what + ", values")
        same(ko[lo + m:hi], (fill if which[i] else k)[lo + m:hi], what + ", keys beyond the count")
        same(vo[lo + m:hi], (fill if which[i] else v)[lo + m:hi], what + ", values beyond the count")
    region = binding.test_scratch_elems(False, pc.ONEPASS_MAX)
    assert not scratch[:region].any(), "the sort left %d words of its one-launch scan region set" % np.count_nonzero(scratch[:region])
    return ko, vo


# (a) sizes on both sides of every edge of the scan's structure x value sets; (f) guard words and zero-after inside run_scans
@pytest.mark.parametrize("values", pc.SCAN_VALUES)
@pytest.mark.parametrize("n", pc.SCAN_SIZES)
def test_scan_sizes_and_values(n, values):
    run_scans([n], [pc.scan_values(values, n)])


# (e) in == out gives the same bytes as two buffers
@pytest.mark.parametrize("n", pc.SCAN_SIZES)
def test_scan_in_place(n):
    a = pc.scan_values("uniform32", n)
    same(run_scans([n], [a], in_place=True), run_scans([n], [a]), "in place against two buffers")


def counted(a, count):
    """the input of a call with a device-side count: nothing beyond the count may be read as data"""
    a = a.copy()
    a[count:] = pc.BEYOND
    return a


# (d) the count on the device, the launch sized by the capacity: both forms of the scan, out of place and in place
@pytest.mark.parametrize("in_place", [False, True], ids=["two_buffers", "in_place"])
@pytest.mark.parametrize("capacity,which", [(cap, i) for cap in (pc.COUNT_CAP_SMALL, pc.COUNT_CAP_SCAN_TWO_LAUNCH) for i in range(8)])
def test_scan_device_count(capacity, which, in_place):
    count = pc.counts_for(capacity)[which]
    a = counted(pc.scan_values("uniform32", capacity), count)
    run_scans([capacity], [a], count=[count], in_place=in_place, count_on_device=True)


# (g) one scratch, zeroed once, scan after scan of either form (the frame's use, and the derived layers' on their shared one)
@pytest.mark.parametrize("sizes", [pc.SCAN_REUSE_ONE_LAUNCH, pc.SCAN_REUSE_TWO_LAUNCH, pc.SCAN_REUSE_MIXED],
                         ids=["one_launch", "two_launch", "mixed"])
@pytest.mark.parametrize("in_place", [False, True], ids=["two_buffers", "in_place"])
def test_scan_reuses_its_scratch(sizes, in_place):
    run_scans(sizes, [pc.scan_values("uniform32", n) for n in sizes], in_place=in_place)


def test_scan_counted_short_of_a_two_launch_scratch():
    """a scratch sized for a two-launch scan, a host-side count that takes the one-launch form (the hooks used to refuse it)"""
    cap = pc.ONEPASS_MAX + 1
    run_scans([cap], [pc.scan_values("uniform32", cap)], count=[pc.TILE])


def test_scan_reuses_its_scratch_with_device_counts():
    """the frontiers' flag scan: one capacity, a count that changes from build to build, zero among them"""
    cap = pc.COUNT_CAP_SMALL
    counts = [cap, 0, pc.TILE + 1, cap + 7, 1, cap - 1]
    a = pc.scan_values("flags", cap)
    run_scans([cap] * len(counts), [counted(a, c) for c in counts], count=counts, count_on_device=True)


# (b) every pass count and every width of the partial top digit, payloads carried / order kept
@pytest.mark.parametrize("vals", ["random", "arange"])
@pytest.mark.parametrize("n", pc.PASS_SIZES)
@pytest.mark.parametrize("nbits", pc.ALL_NBITS)
def test_sort_every_key_width(nbits, n, vals):
    v = pc.random_vals(n) if vals == "random" else np.arange(n, dtype=np.uint32)
    run_sorts([n], nbits, [pc.uniform_keys(n, nbits)], [v])


@pytest.mark.parametrize("nbits", pc.VOXEL_NBITS)
def test_sort_voxel_like_keys(nbits):
    n = pc.VOXEL_N
    run_sorts([n], nbits, [pc.voxel_like_keys(n, nbits)], [np.arange(n, dtype=np.uint32)])


@pytest.mark.parametrize("nbits,shape", [(b, s) for b in pc.SHAPE_NBITS for s in pc.SHAPES
                                         if pc.shaped_keys(s, pc.SHAPE_N, b) is not None])
def test_sort_shaped_keys(nbits, shape):
    n = pc.SHAPE_N
    run_sorts([n], nbits, [pc.shaped_keys(shape, n, nbits)], [np.arange(n, dtype=np.uint32)])


# (c) sizes, up to both sides of the histogram scan's switch to two launches
@pytest.mark.parametrize("nbits", pc.SORT_SIZE_NBITS)
@pytest.mark.parametrize("n", pc.SORT_SIZES)
def test_sort_sizes(n, nbits):
    run_sorts([n], nbits, [pc.uniform_keys(n, nbits)], [pc.random_vals(n)])


# (d) the count on the device: a result that lands in the first pair (two passes) and in the second (three)
@pytest.mark.parametrize("capacity,nbits,which",
                         [(pc.COUNT_CAP_SMALL, b, i) for b in (16, 25) for i in range(8)]
                         + [(pc.COUNT_CAP_SORT_TWO_LAUNCH, 25, i) for i in range(8)])
def test_sort_device_count(capacity, nbits, which):
    count = pc.counts_for(capacity)[which]
    keys, vals = counted(pc.uniform_keys(capacity, nbits), count), counted(pc.random_vals(capacity), count)
    run_sorts([capacity], nbits, [keys], [vals], count=[count], count_on_device=True)


# (h) one scratch, zeroed once, sort after sort with both forms of the histogram scan (the map's frame-after-frame use)
def test_sort_reuses_its_scratch():
    sizes, nbits = pc.SORT_REUSE, pc.SORT_REUSE_NBITS
    run_sorts(sizes, nbits, [pc.uniform_keys(n, nbits) for n in sizes], [pc.random_vals(n) for n in sizes])


def test_sort_reuses_its_scratch_with_device_counts():
    cap = pc.COUNT_CAP_SMALL
    counts = [cap, 0, pc.TILE + 1, cap + 7, 1, cap - 1]
    nbits = [25, 25, 16, 28, 7, 19]
    keys = [counted(pc.uniform_keys(cap, b), c) for b, c in zip(nbits, counts)]
    vals = [counted(pc.random_vals(cap), c) for c in counts]
    run_sorts([cap] * len(counts), nbits, keys, vals, count=counts, count_on_device=True)
