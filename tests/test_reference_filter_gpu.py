"""The HIP library against the reference's own filter, directly - not through the oracle.

tests/golden/ref_filter_<variant>.npz holds what the reference's updateParticles, birth members and
resampleParticlesInVoxel (semantic_dsp_map.h, compiled over oracle/ref_shims/ and driven by oracle/ref_filter_harness.cpp)
answered to the scenarios of tests/ref_filter_cases.py.  The library runs the frames of the two small variants (t1: 64 x
32 x 64 voxels, 4 slots, 192 x 108; t0: 32^3, 8 slots, 128 x 80; both with the reference's 7 x 7 window) through
load_state, set_ring_state (with birth_cursor), set_stamps and update(stop_after="weight" | "birth"), and is compared
through dump_state (the owner field included), ring_state, stats, object_particle_count and tracks_with_particles.

Exact scenarios (weight_single_*, birth_*, cursor_wrap, two_frames) are compared bit for bit.  In weight_window_edges,
weight_forget* and weight_random_* the integers are exact - the reference's own three summation orders agree on every one of them, so
nothing is left out - and the weights are within 4 x the largest relative difference among those three orders
(ref_filter_cases.MEASURED_ORDER_SPREAD; the library's row partial sums are a fourth order), floored at one ulp of the
largest weight and never looser than the 1e-4 of tests/test_parity_gpu.py.  ck_kappa has no reference value (a local of
updateParticles that the harness does not recompute); tests/test_parity_gpu.py holds it.  resample_direct and guessed
are direct calls that the library has no entry point for; the birth scenarios reach the resampling through a frame.
Nothing of the reference is read here: the fixtures and the checkout are enough.
"""
import functools
import os

import numpy as np
import pytest

from oracle import ref_filter
from semantic_dsp_map_amd import binding
from tests import ref_filter_cases as fc
from tests import ref_ring_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("t1", "t0")


@functools.lru_cache(maxsize=None)
def scenarios(variant):
    return {sc["name"]: sc for sc in fc.scenarios(variant)}


@functools.lru_cache(maxsize=None)
def records(variant, name, key=""):
    with np.load(os.path.join(GOLDEN, "ref_filter_%s.npz" % variant)) as z:
        return ref_filter.parse(z[name + ".out" + key].tobytes().decode("ascii"))


def make(cfg, params, noise):
    return binding.SdmMap(cfg, params, noise)


@pytest.mark.parametrize("name", fc.GPU_FRAMES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_frame(variant, name):
    """the weight stage, and where the scenario has births the birth stage, each as a frame stopped after it on a map put
    into the state the reference was in"""
    sc, rec = scenarios(variant)[name], records(variant, name)
    tol = None if sc["exact"] else fc.weight_tol(variant, name)
    m = fc.run_frame(make, sc, rec, "weight")
    ref_bins = {p: np.sort(b) for p, b in ref_filter.first(rec, "bins").items()}      # the library's canonical order
    rc.check_bins(ref_bins, rc.split_bins(m), name, ordered=True)
    fc.check_particles(sc, ref_filter.first(rec, "particles", 0), m.dump_state(), name + " after the weight stage", tol=tol)
    assert m.ring_state()["global_time_stamp"] == sc["ts"] and m.ring_state()["birth_cursor"] == sc["burn"]
    if sc["births"]:
        m = fc.run_frame(make, sc, rec, "birth")
        fc.check_births(sc, rec, m, name)
        own = {t: v for t, v in ref_filter.first(rec, "owners").items() if len(v)}
        assert m.tracks_with_particles().tolist() == sorted(own)
        for t in list(own) + [fc.STATIC_A, fc.STATIC_B, 9]:
            assert m.object_particle_count(t) == len(own.get(t, ())), "track %d" % t


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_frames(variant):
    """two consecutive frames with the move of an object between them: the noise cursor and the owner sets carried over
    (ref_filter_cases.check_two_frames has the one recorded deviation, the slot order of an object's moved particles)"""
    sc = scenarios(variant)["two_frames"]
    rec = records(variant, "two_frames")
    m = fc.run_two_frames(make, sc, rec)
    fc.check_two_frames(sc, rec, records(variant, "two_frames", "c"), m, "two_frames")
    own = {t: v for t, v in ref_filter.first(records(variant, "two_frames", "c"), "owners", 1).items() if len(v)}
    assert m.tracks_with_particles().tolist() == sorted(own)
    for t in own:
        assert m.object_particle_count(t) == len(own[t]), "track %d" % t
