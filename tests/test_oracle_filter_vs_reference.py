"""The CPU oracle against the reference's own filter (CPU only).

tests/golden/ref_filter_<variant>.npz holds, per scenario of tests/ref_filter_cases.py, the commands that were given to
oracle/ref_filter_harness.cpp - SemanticDSPMap::updateParticles, addGuessedParticle, addNewbornParticleAndResample,
addNewbornParticleWithNoiseAndResample and resampleParticlesInVoxel of the reference's semantic_dsp_map.h over its
ObjectParticleHashMap, compiled as they stand over the stand-in headers of oracle/ref_shims/ - and the text it answered.
Here the oracle runs the same scenarios with bin_order=0, the reference's own order of operations, and every float is
compared bit for bit and every integer exactly: status, stamp, forget count, track, label, slot, the noise cursor, the
owner sets, the return values of the resampling and the number of particles added.  No tolerance is in play: the -O0 /
-O3 spread of the harness is zero (ref_filter_cases.MEASURED_SPREAD).

Not compared: ck_kappa.  The reference keeps it in a local array (semantic_dsp_map.h:973) that the harness cannot read
and does not recompute; every weight it answers is a function of it, and tests/test_parity_gpu.py and the known-answer
tests hold the array itself.  The order in which the births visit the pixels is the harness's own reading of lines
777-800 (that loop sits in a member that needs PCL), pinned by reading, not by compilation.

Where oracle/_ref/ holds the harness executables (`make -C oracle ref`, which needs the reference), every scenario is
run again and must reproduce the fixture byte for byte; only that leg may skip.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import ref_filter
from tests import ref_filter_cases as fc
from tests import ref_ring_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def scenarios(variant):
    return {sc["name"]: sc for sc in fc.scenarios(variant)}


@functools.lru_cache(maxsize=None)
def fixture(variant):
    with np.load(os.path.join(GOLDEN, "ref_filter_%s.npz" % variant)) as z:
        return {k: z[k].tobytes().decode("ascii") for k in z.files}


@functools.lru_cache(maxsize=None)
def records(variant, name, key=""):
    return ref_filter.parse(fixture(variant)[name + ".out" + key])


CASES = [(v, n) for v in ref_filter.VARIANTS for n in fc.NAMES]
case = pytest.mark.parametrize("variant,name", CASES, ids=["%s-%s" % c for c in CASES])


def make(cfg, params, noise):
    return orc.OracleMap(cfg, params, noise)


def test_names_cover_the_scenarios():
    for variant in ref_filter.VARIANTS:
        assert list(scenarios(variant)) == fc.NAMES
        assert sorted(k.split(".")[0] for k in fixture(variant) if k.endswith(".cmd")) == sorted(fc.NAMES)


@case
def test_fixture_is_of_this_scenario(variant, name):
    """the commands stored beside the reference's answer are the ones today's scenario builder writes"""
    sc = scenarios(variant)[name]
    assert fc.scripts(sc)[""] == fixture(variant)[name + ".cmd"]
    v = ref_filter.first(records(variant, name), "variant")
    cfg = fc.config(variant)
    assert v["n"] == list(rc.dims(cfg)[0]) and v["slots"] == rc.dims(cfg)[1] and (v["width"], v["height"]) == (cfg["width"], cfg["height"])
    assert cfg["window_half"] == fc.window_half(variant)


@case
def test_harness_reproduces_fixture(variant, name):
    path = ref_filter.exe(variant)
    if not os.path.exists(path):
        pytest.skip("no reference harness: %s is missing (make -C oracle ref, with the reference at hand)" % path)
    fx = fixture(variant)
    answers = {k[len(name) + 4:]: v for k, v in fx.items() if k.startswith(name + ".out")}
    for key, text in fc.scripts(scenarios(variant)[name], answers).items():
        assert ref_filter.run(variant, text) == fx[name + ".out" + key], "the harness no longer answers as recorded"


@pytest.mark.parametrize("variant", list(ref_filter.VARIANTS))
def test_order_spread_is_as_recorded(variant):
    """MEASURED_ORDER_SPREAD is what the reference's own three summation orders give, the integers never depend on the
    order (so no particle is left out of a comparison: the ambiguous share is 0), and 4 x the spread stays under 1e-4"""
    for name, want in fc.MEASURED_ORDER_SPREAD[variant].items():
        recs = [records(variant, name, k) for k in ("", "o1", "o2")]
        worst, differ = fc.order_spread(recs)
        print("%s %s: order spread %.3e, tolerance %.3e, integers that differ %d" % (variant, name, worst, fc.weight_tol(variant, name), len(differ)))
        assert worst == want, (variant, name, worst)
        assert len(differ) / len(ref_filter.first(recs[0], "particles", 0)["idx"]) <= fc.AMBIGUOUS_CAP and not differ
        assert fc.weight_tol(variant, name) <= fc.ORDER_CAP


@case
def test_oracle_matches_reference(variant, name):
    sc, rec = scenarios(variant)[name], records(variant, name)
    if sc["kind"] == "resample":
        m = fc.make_map(make, sc, rec, sc["ts"])
        got = np.array([m.resample_voxel(int(v)) for v in sc["voxels"]], np.uint8)
        ref = ref_filter.first(rec, "resample")
        assert np.array_equal(ref, got), (ref, got)
        assert ref[0] == 0 and ref[1:].all(), "exactly S/2 UPDATED particles must not resample, S/2 + 1 must: %s" % ref
        st = m.dump_state()
        fc.check_particles(sc, ref_filter.first(rec, "particles"), st, name)
        fc.check_owners(ref_filter.first(rec, "owners"), st, name)
        fc.assert_resample_cases(sc, ref_filter.first(rec, "particles"))
    elif sc["kind"] == "guessed":
        m = fc.make_map(make, sc, rec, sc["ts"])
        for label, track, pts in sc["groups"]:
            for p in pts:
                m.add_guessed_point(*p, label=label, track=track)
        st = m.dump_state()
        fc.check_particles(sc, ref_filter.first(rec, "particles"), st, name)
        fc.check_owners(ref_filter.first(rec, "owners"), st, name)
        own = {t: v for t, v in ref_filter.first(rec, "owners").items() if len(v)}
        assert sorted(own) == [5, 7, fc.MAX_MOVABLE] and len(own[5]) == 3, own       # the full voxel refused one; static tracks own nothing
    elif sc["kind"] == "two_frames":
        fc.check_two_frames(sc, rec, records(variant, name, "c"), fc.run_two_frames(make, sc, rec), name)
    else:
        m = fc.run_frame(make, sc, rec, "weight")
        rc.check_bins(ref_filter.first(rec, "bins"), rc.split_bins(m), name, ordered=True)
        fc.check_particles(sc, ref_filter.first(rec, "particles", 0), m.dump_state(), name + " after the weight stage")
        fc.assert_weight_cases(sc, rec)
        if sc["births"]:
            m = fc.run_frame(make, sc, rec, "birth")
            fc.check_births(sc, rec, m, name)
            fc.assert_birth_cases(sc, rec)
