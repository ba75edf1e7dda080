"""The HIP library against the reference's own ring buffer, directly - not through the oracle.

tests/golden/ref_ring_<variant>.npz holds what the reference's mc_ring/*.h (compiled over oracle/ref_shims/, driven by
oracle/ref_harness.cpp) answered to the scenarios of tests/ref_ring_cases.py.  The library runs the scenarios of the two
small variants (t1: 64 x 32 x 64 voxels, 4 slots, 192 x 108; t0: 32^3, 8 slots, 128 x 80) through load_state,
set_ring_state, set_stamps and update(stop_after), and is compared as tests/test_oracle_vs_reference.py compares the
oracle: integers exactly, the floats of exact scenarios bit for bit, those of random ones within FLOAT_TOL, ambiguous
points left out.  The per-pixel lists are compared in ascending index order, the library's canonical order; the
reference's own push order is checked on the CPU against the oracle with bin_order=0.  Nothing of the reference is
read here: the fixtures and the checkout are enough.
"""
import functools
import os

import numpy as np
import pytest

from oracle import ref_ring
from semantic_dsp_map_amd import binding
from tests import ref_ring_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("t1", "t0")
FRAMES = ["insert", "move_exact", "move_overflow", "move_random", "visible_z", "visible_back", "visible_oblique", "occupancy_exact",
          "wsum_exact", "occupancy_random", "wsum_random"]
EGO = ["ego_axes", "ego_wrap", "ego_random"]


@functools.lru_cache(maxsize=None)
def scenarios(variant):
    return {sc["name"]: sc for sc in rc.scenarios(variant)}


@functools.lru_cache(maxsize=None)
def records(variant, name, key=""):
    with np.load(os.path.join(GOLDEN, "ref_ring_%s.npz" % variant)) as z:
        return ref_ring.parse(z[name + ".out" + key].tobytes().decode("ascii"))


def make(cfg, params, noise):
    return binding.SdmMap(cfg, params, noise)


@pytest.mark.parametrize("name", EGO)
@pytest.mark.parametrize("variant", VARIANTS)
def test_ego_shift(variant, name):
    """updateEgoCenterPos / updateRingbufferIndexParams (operations.h:68-96, 1111-1191): steps, offsets, map centre and
    the stamps of the recycled slabs after every step of a path"""
    sc, rec = scenarios(variant)[name], records(variant, name)
    for k, (ring, stamps) in enumerate(rc.run_ego(make, sc)):
        rc.check_ring(ref_ring.first(rec, "ring", k), ring, "%s step %d" % (name, k))
        rc.check_stamps(ref_ring.first(rec, "stamps", k), stamps, "%s step %d" % (name, k))


@pytest.mark.parametrize("variant", VARIANTS)
def test_position_to_voxel(variant):
    """globalFramePostoVoxelIdx (operations.h:841-883) on a shifted ring, through the point query's storage index"""
    sc, rec = scenarios(variant)["index"], records(variant, "index")
    m = rc.make_map(make, sc)
    m.set_ring_state(rc.ring_dict(ref_ring.first(rec, "ring"), len(sc["path"])))
    _, got = m.query_points(sc["points"], with_index=True)
    ref = ref_ring.first(rec, "pos_to_voxel")
    keep = ~sc["ambiguous"]
    assert np.array_equal(ref[keep], got[keep]), np.flatnonzero(keep & (ref != got))[:8]


@pytest.mark.parametrize("name", FRAMES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_frame(variant, name):
    """insertion, object moves, removal, the visibility BFS and the occupancy fusion, each as a frame stopped after its
    stage on a map put into the state the reference was in"""
    sc, rec = scenarios(variant)[name], records(variant, name)
    rc.check_frame(sc, rec, rc.run_frame(make, sc, rec), bins_ordered=False)


def test_pdf_table():
    """standard_gaussian_pdf as calculateGaussianTable fills it (basic_algorithms.h:405-407, 456-460)"""
    ref = ref_ring.first(records("t1", "tables"), "pdf_table")
    m = binding.SdmMap(rc.config("t1"), rc.PARAMS, np.zeros(8, np.float32))
    assert np.array_equal(rc.bits(ref), rc.bits(m.download_pdf_table()))
