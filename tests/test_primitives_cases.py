"""CPU checks of tests/primitives_cases.py, the ground the device tests of the scan and the sort stand on: the key
generators reach every digit of every pass, the voxel-like keys hold the long off-tile runs, the wrapping inputs do wrap,
the size tables straddle every edge they are there for; and the sequence hooks refuse what they must before they touch a
GPU."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import primitives_cases as pc


@pytest.mark.parametrize("n", pc.PASS_SIZES)
@pytest.mark.parametrize("nbits", pc.ALL_NBITS)
def test_uniform_keys_reach_every_digit(n, nbits):
    k = pc.uniform_keys(n, nbits)
    assert k.dtype == np.uint32 and k.size == n and not k.flags.writeable
    assert int(k.max()) < (1 << nbits)
    ds = pc.digits(k, nbits)
    assert len(ds) == pc.sort_passes(nbits)
    for d in ds:
        assert np.unique(d).size > 1
    # the top digit is partial unless nbits is a whole number of digits: its highest bit is used
    assert int(k.max()) >> (nbits - 1) == 1


@pytest.mark.parametrize("nbits", pc.VOXEL_NBITS)
def test_voxel_like_keys_hold_long_runs_off_the_tile_edges(nbits):
    n = pc.VOXEL_N
    assert n % pc.TILE != 0
    k = pc.voxel_like_keys(n, nbits)
    sentinel = 1 << (nbits - 1)
    assert k.size == n and int(k.max()) == sentinel            # inside the precondition keys < 2^nbits
    assert 0.25 < np.mean(k == sentinel) < 0.75
    start, length = pc.equal_runs(k)
    real = k[start] != sentinel
    off_tile = start % pc.TILE != 0
    assert np.any(real & off_tile & (length > pc.LANES) & (length <= pc.TILE))
    assert np.any(real & off_tile & (length > pc.TILE))
    assert np.any(real & (length <= 3))
    # a run longer than a tile crosses a tile edge whatever its start
    long_run = np.flatnonzero(real & (length > pc.TILE))[0]
    assert start[long_run] // pc.TILE != (start[long_run] + length[long_run] - 1) // pc.TILE


@pytest.mark.parametrize("nbits", pc.SHAPE_NBITS)
def test_shaped_keys_are_what_they_say(nbits):
    n = pc.SHAPE_N
    top = (1 << nbits) - 1
    for shape in pc.SHAPES:
        k = pc.shaped_keys(shape, n, nbits)
        if k is None:
            assert shape == "middle_digit" and pc.sort_passes(nbits) < 3
            continue
        assert k.size == n and int(k.max()) <= top
        ds = [np.unique(d).size for d in pc.digits(k, nbits)]
        if shape in ("all_equal", "all_max"):
            assert ds == [1] * len(ds) and (shape == "all_equal" or int(k[0]) == top)
        elif shape == "sorted":
            assert np.all(k[1:] >= k[:-1]) and k[0] != k[-1]
        elif shape == "reversed":
            assert np.all(k[1:] <= k[:-1]) and k[0] != k[-1]
        elif shape == "top_digit":
            assert ds[-1] > 1 and ds[:-1] == [1] * (len(ds) - 1)
        else:
            varying = [i for i, c in enumerate(ds) if c > 1]
            assert len(varying) == 1 and 0 < varying[0] < len(ds) - 1
    assert any(pc.shaped_keys("middle_digit", n, b) is not None for b in pc.SHAPE_NBITS)


def test_wrapping_scan_inputs_wrap():
    for n in pc.SCAN_SIZES:
        a = pc.scan_values("uniform32", n)
        if n >= pc.ITEMS:
            assert int(a.astype(np.uint64).sum()) > 1 << 32
        assert int(pc.scan_values("small", n).max()) <= 8
        f = pc.scan_values("flags", n)
        on = np.flatnonzero(f)
        assert set(np.unique(f)) <= {0, 1} and np.all((on % pc.TILE == 0) | (on % pc.TILE == pc.TILE - 1))
        assert on.size == n // pc.TILE + (n + pc.TILE - 1) // pc.TILE
    n = 2 * pc.TILE + 1
    assert int(pc.scan_values("all_ones", n).astype(np.uint64).sum()) > 1 << 32


def test_references():
    a = np.array([0xFFFFFFFF, 2, 0xFFFFFFFF, 5], np.uint32)
    assert pc.scan_ref(a).tolist() == [0, 0xFFFFFFFF, 1, 0]
    assert pc.scan_ref(a, 2).tolist() == [0, 0xFFFFFFFF] and pc.scan_ref(a, 0).size == 0
    big = pc.scan_values("uniform32", 100000)
    want = [sum(int(v) for v in big[:i]) % (1 << 32) for i in (0, 1, 2, 77777, 99999)]
    assert pc.scan_ref(big)[[0, 1, 2, 77777, 99999]].tolist() == want
    t = pc.tile_totals_ref(big, 5000, 100000)
    assert t.size == pc.tiles(100000) and not t[3:].any()
    assert t[:3].tolist() == [sum(int(v) for v in big[i * pc.TILE:min((i + 1) * pc.TILE, 5000)]) % (1 << 32) for i in range(3)]
    k = np.array([3, 1, 3, 0, 1], np.uint32)
    assert pc.sort_ref(k).tolist() == [3, 1, 4, 0, 2]


def test_size_tables_straddle_every_edge():
    s = set(pc.SCAN_SIZES)
    for edge in (pc.ITEMS, pc.LANES, pc.TILE, 2 * pc.TILE, pc.ONEPASS_MAX):
        assert {edge - 1, edge, edge + 1} <= s
    assert pc.one_launch(pc.ONEPASS_MAX) and not pc.one_launch(pc.ONEPASS_MAX + 1)
    assert any(pc.tiles(n) > 256 + 1 and not pc.one_launch(n) for n in s)     # the strided loop over predecessors' totals
    assert all(pc.one_launch(n) for n in pc.SCAN_REUSE_ONE_LAUNCH) and pc.ONEPASS_MAX in pc.SCAN_REUSE_ONE_LAUNCH
    assert not any(pc.one_launch(n) for n in pc.SCAN_REUSE_TWO_LAUNCH)
    assert pc.SCAN_REUSE_ONE_LAUNCH == [2049, 1, 512 * 2048, 65, 512 * 2048, 4097]
    assert pc.SCAN_REUSE_TWO_LAUNCH == [512 * 2048 + 1, 4194321, 512 * 2048 + 1]
    assert pc.SCAN_REUSE_MIXED == [512 * 2048 + 1, 2049, 4194321, 512 * 2048, 1, 512 * 2048 + 1]
    forms = [pc.one_launch(n) for n in pc.SCAN_REUSE_MIXED]
    assert sum(a != b for a, b in zip(forms, forms[1:])) >= 3 and not forms[0] and not forms[-1]
    t = set(pc.SORT_SIZES)
    for edge in (pc.LANES, 256, pc.TILE):
        assert {edge - 1, edge, edge + 1} <= t
    # the sort's histogram scan: 512 counters per tile of keys
    hist = lambda n: pc.tiles(n) << pc.RADIX_BITS
    assert pc.one_launch(hist(pc.SORT_ONEPASS_MAX)) and not pc.one_launch(hist(pc.SORT_ONEPASS_MAX + 1))
    assert {pc.SORT_ONEPASS_MAX, pc.SORT_ONEPASS_MAX + 1} <= t and pc.SORT_ONEPASS_MAX == 2048 * 2048
    assert pc.SORT_REUSE == [2048 * 2048 + 1, 2049, 2048 * 2048 + 1, 1, 300000]
    assert [pc.one_launch(hist(n)) for n in pc.SORT_REUSE] == [False, True, False, True, True]
    assert {pc.sort_passes(b) for b in pc.VOXEL_NBITS} == {1, 2, 3, 4} and {pc.sort_passes(b) for b in pc.ALL_NBITS} == {1, 2, 3, 4}
    assert pc.one_launch(pc.COUNT_CAP_SMALL) and not pc.one_launch(pc.COUNT_CAP_SCAN_TWO_LAUNCH)
    assert not pc.one_launch(hist(pc.COUNT_CAP_SORT_TWO_LAUNCH))
    for cap in (pc.COUNT_CAP_SMALL, pc.COUNT_CAP_SCAN_TWO_LAUNCH, pc.COUNT_CAP_SORT_TWO_LAUNCH):
        assert pc.counts_for(cap) == [0, 1, 2047, 2048, 2049, cap - 1, cap, cap + 7]


def test_hooks_refuse_bad_sequences_before_touching_a_gpu():
    """the argument checks of the sequence hooks come before their first HIP call: a host-side count fits its capacity,
    nbits is 1..32.  (Sequences that mix the two forms of the scan are no longer refused: they work,
    tests/test_primitives_gpu.py::test_scan_reuses_its_scratch and ::test_scan_counted_short_of_a_two_launch_scratch.)"""
    z = lambda n: np.zeros(n, np.uint32)
    with pytest.raises(binding.SdmError, match="SDM_ERR_INVALID_ARGUMENT"):
        binding.test_scan_seq([8], z(8), z(8), count=[9])
    for nbits in (0, 33):
        with pytest.raises(binding.SdmError, match="SDM_ERR_INVALID_ARGUMENT"):
            binding.test_sort_pairs_seq([8], nbits, z(8), z(8), z(8), z(8))
    # what the scratch sizes say about the two forms, as far as the tests rely on it: the sort's scratch starts with
    # room for the longest one-launch scan
    assert binding.test_scratch_elems(True, 1) > binding.test_scratch_elems(False, pc.ONEPASS_MAX)
