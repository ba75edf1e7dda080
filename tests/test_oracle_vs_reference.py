"""The CPU oracle against the reference's own ring buffer (CPU only).

tests/golden/ref_ring_<variant>.npz holds, per scenario of tests/ref_ring_cases.py, the commands that were given to
oracle/ref_harness.cpp - the reference's mc_ring/*.h compiled over the stand-in headers of oracle/ref_shims/ - and the
text it answered.  Here the oracle runs the same scenarios through update(stop_after), load_state, set_ring_state,
set_stamps and its known-answer helpers, with bin_order=0 (the literal BFS order), and is compared with those answers:
integers exactly, the floats of exact scenarios bit for bit, the floats of random ones within ref_ring_cases.FLOAT_TOL.
This pins the ring layer (ego shift, index math, slot choice, moves, removal, visibility BFS, frustum, occupancy
fusion) and the tables; generateLabeledPointCloud is held the same way by tests/test_oracle_cloud_vs_reference.py;
SemanticDSPMap::subObjectLevelUpdate itself and object_layer.h stay unpinned.

Where oracle/_ref/ holds the harness executables (`make -C oracle ref`, which needs the reference), every scenario is
run again and must reproduce the fixture byte for byte; only that leg may skip.

Recorded deviations, each with its own branch below:
  * move_overflow: the one place where the oracle knowingly departs from the reference - an object's index set is
    walked in ascending order, not std::unordered_set order, so when more particles of ONE object land in a voxel than
    fit, which of them survive may differ.  The scenario gives the object's particles the same weight, label and
    forget count, so the multiset of the survivors' fields other than position does not depend on that order and is
    asserted equal in full; every survivor's position must be one of the object's moved positions, none twice; every
    other voxel is compared slot by slot.
  * bfs_limits: a BFS start vertex outside the vertex grid is undefined behaviour in the reference (unchecked index),
    so the harness refuses to run it, and for the multi-threaded BFS that is every view of these variants.  This case
    only asserts what the harness recorded (refused, refused, ran); it runs neither the oracle nor the library, and
    covers neither.  The oracle's own early return for such a start (cpu_ref.cpp, visibility) cannot be reached
    through update(), which puts the camera at the ego position, inside the grid; it stays untested.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import ref_ring
from tests import ref_ring_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def scenarios(variant):
    return {sc["name"]: sc for sc in rc.scenarios(variant)}


@functools.lru_cache(maxsize=None)
def fixture(variant):
    with np.load(os.path.join(GOLDEN, "ref_ring_%s.npz" % variant)) as z:
        return {k: z[k].tobytes().decode("ascii") for k in z.files}


@functools.lru_cache(maxsize=None)
def records(variant, name, key=""):
    return ref_ring.parse(fixture(variant)[name + ".out" + key])


# the names are spelled out so that collection does not build the scenarios
NAMES = ["ego_axes", "ego_wrap", "ego_random", "index", "insert", "guessed_add", "move_exact", "move_overflow", "move_random", "visible_z",
         "visible_back", "visible_oblique", "occupancy_exact", "wsum_exact", "occupancy_random", "wsum_random", "neighbours",
         "frustum", "bfs_limits"]
CASES = [(v, n) for v in ref_ring.VARIANTS for n in NAMES] + [("t1", "tables")]
case = pytest.mark.parametrize("variant,name", CASES, ids=["%s-%s" % c for c in CASES])


def make(cfg, params, noise):
    return orc.OracleMap(cfg, params, noise)


def test_names_cover_the_scenarios():
    for variant in ref_ring.VARIANTS:
        assert sorted(scenarios(variant)) == sorted(n for v, n in CASES if v == variant)
        assert sorted(k.split(".")[0] for k in fixture(variant) if k.endswith(".cmd")) == sorted(scenarios(variant))


@case
def test_fixture_is_of_this_scenario(variant, name):
    """the commands stored beside the reference's answer are the ones today's scenario builder writes"""
    sc = scenarios(variant)[name]
    assert rc.script(sc) == fixture(variant)[name + ".cmd"]
    v = ref_ring.first(records(variant, name), "variant")
    cfg = rc.config(variant)
    assert v["n"] == list(rc.dims(cfg)[0]) and v["slots"] == rc.dims(cfg)[1] and (v["width"], v["height"]) == (cfg["width"], cfg["height"])
    cam = ref_ring.first(records(variant, name), "camera")
    want = np.array([cfg[k] for k in ("voxel_size", "fx", "fy", "cx", "cy", "depth_min", "depth_max")], np.float32)
    assert np.array_equal(cam, want), (cam, want)


@case
def test_ambiguous_share_is_capped(variant, name):
    assert rc.ambiguous_share(scenarios(variant)[name]) <= rc.AMBIGUOUS_CAP


@case
def test_harness_reproduces_fixture(variant, name):
    path = ref_ring.exe(variant)
    if not os.path.exists(path):
        pytest.skip("no reference harness: %s is missing (make -C oracle ref, with the reference at hand)" % path)
    fx = fixture(variant)
    for key in ("", "2"):
        if name + ".cmd" + key in fx:
            assert ref_ring.run(variant, fx[name + ".cmd" + key]) == fx[name + ".out" + key], "the harness no longer answers as recorded"


@case
def test_oracle_matches_reference(variant, name):
    sc = scenarios(variant)[name]
    cfg = rc.config(variant)
    rec = records(variant, name)
    kind = sc["kind"]
    if kind == "ego":
        got = rc.run_ego(make, sc)
        for k, (ring, stamps) in enumerate(got):
            rc.check_ring(ref_ring.first(rec, "ring", k), ring, "%s step %d" % (name, k))
            rc.check_stamps(ref_ring.first(rec, "stamps", k), stamps, "%s step %d" % (name, k))
    elif kind == "index":
        m = rc.make_map(make, sc)
        m.set_ring_state(rc.ring_dict(ref_ring.first(rec, "ring"), len(sc["path"])))
        ref_v = ref_ring.first(rec, "pos_to_voxel")
        got_v = np.array([m.pos_to_voxel(*p) for p in sc["points"]], np.uint32)
        keep = ~sc["ambiguous"]
        assert np.array_equal(ref_v[keep], got_v[keep]), np.flatnonzero(keep & (ref_v != got_v))[:8]
        assert (ref_v == 0xffffffff).any() and (ref_v != 0xffffffff).sum() > 100
        voxels = np.unique(ref_v[ref_v != 0xffffffff])
        ref_p = ref_ring.first(records(variant, name, "2"), "voxel_to_pos")
        got_p = np.array([m.voxel_to_pos(int(v)) for v in voxels], np.float32)
        assert np.array_equal(rc.bits(ref_p), rc.bits(got_p))
    elif kind == "adds":
        m = rc.make_map(make, sc)
        m.set_ring_state(rc.ring_dict(ref_ring.first(rec, "ring"), sc["ts"]))
        got = np.array([m.add_guessed_particle(*p, label=sc["label"], track=sc["track"]) for p in sc["points"]], np.uint32)
        ref = ref_ring.first(rec, "add")[:, 1]
        assert np.array_equal(ref, got), (ref, got)
        assert (ref == 0xffffffff).sum() >= 3 and (ref != 0xffffffff).sum() == rc.dims(cfg)[1]     # full, on map_p_max, outside
        rc.check_state(sc, ref_ring.first(rec, "state"), m.dump_state(), name)
    elif kind == "tables":
        m = orc.OracleMap(dict(cfg, bin_order=0), rc.PARAMS, np.zeros(8, np.float32))
        assert np.array_equal(rc.bits(ref_ring.first(rec, "pdf_table")), rc.bits(m.pdf_table()))
        got = np.array([m.query_pdf(*q) for q in sc["queries"]], np.float32)
        assert np.array_equal(rc.bits(ref_ring.first(rec, "query_pdf")), rc.bits(got))
        got = np.array([m.forgetting_factor(c) for c in sc["forgetting"][2]], np.float32)
        assert np.array_equal(rc.bits(ref_ring.first(rec, "forgetting_factor")), rc.bits(got))
    elif kind == "frustum":
        depth, cloud = rc.blank(cfg)
        for k, view in enumerate(sc["views"]):
            m = rc.make_map(make, sc)
            m.update(depth, cloud, view["pos"], view["q"], stop_after="visibility")
            got = np.array([m.point_in_frustum(*p) for p in view["points"]], np.uint8)
            ref = ref_ring.first(rec, "frustum", k)
            keep = ~view["ambiguous"]
            assert np.array_equal(ref[keep], got[keep]), np.flatnonzero(keep & (ref != got))[:8]
            assert 0.1 < ref.mean() < 0.9, "the view tests nothing: %f of its points are inside" % ref.mean()
    elif kind == "bfs_limits":
        # recorded deviation: the reference cannot run these (undefined behaviour), so only the harness's record is
        # checked here and neither the oracle nor the library runs; see the module docstring
        flags = [v for n, v in rec if n == "visible"]
        assert flags == [0, 0, 1], flags        # start outside the map; multi-threaded from the map centre; single-threaded from there
    else:
        rc.check_frame(sc, rec, rc.run_frame(make, sc, rec), bins_ordered=True)


def test_insert_takes_the_slots_the_scenario_is_built_for():
    """the cases of the insertion scenario are what their comments say: what the reference answered is the slot each was
    built to get (first vacant, stale slots reused, full and outside rejected)"""
    for variant in ref_ring.VARIANTS:
        sc = scenarios(variant)["insert"]
        adds = [v for n, v in records(variant, "insert") if n == "add"]
        got = [None if a[0, 1] == 0xffffffff else int(a[0, 1]) for a in adds]
        assert got == sc["expect_slots"], (variant, got, sc["expect_slots"])
        assert None in got and len([g for g in got if g is not None]) >= 8


def test_move_scenarios_hit_their_cases():
    for variant in ref_ring.VARIANTS:
        sets = ref_ring.first(records(variant, "move_exact"), "move")
        sc = scenarios(variant)["move_exact"]
        sp = sc["state"]
        before = [int((sp["owner"] == t).sum()) for t, _ in sc["moves"] if (sp["owner"] == t).any()]
        after = [len(x) for x in sets]
        assert before == [5, 3, 2, 1] and after == [5, 3, 0, 0], (variant, before, after)     # out of the map; into a full voxel
        s = rc.dims(rc.config(variant))[1]
        assert len(set(int(i) // s for i in sets[0]) & set(int(i) // s for i in sets[1])) == 1   # two objects meet in one voxel
