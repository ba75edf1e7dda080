"""The CPU oracle's generate_cloud_ex against the reference's own generateLabeledPointCloud (CPU only).

tests/golden/ref_cloud_<variant>.npz holds, per scenario of tests/ref_cloud_cases.py, what oracle/ref_cloud_harness.cpp -
utils/pointcloud_tools.h:88-310 and 1104-1133 compiled as they stand over the stand-in headers of oracle/ref_shims/ -
answered, and the hash of the scenario file it was given.  The inputs are regenerated here from their seeds; the oracle
is configured from the record (camera, depth range, largest movable id, Sky's instance, label tables) and compared
under the rules stated in tests/ref_cloud_cases.py.

Where oracle/_ref/ holds the harness executables (`make -C oracle ref`, which needs the reference), every scenario is
run again and must reproduce the fixture byte for byte; only that leg may skip.

Recorded deviation with its own branch: the adapter's label table gives 65535 (Background's instance)
to a static-mask value whose label has no static instance, where the reference's default insertion gives 0;
test_adapter_table_against_the_record states exactly that difference and nothing else.
"""
import functools
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import ref_cloud
from semantic_dsp_map_amd import synth
from tests import ref_cloud_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def scenario(variant, name):
    return cc.scenario(variant, name)


@functools.lru_cache(maxsize=None)
def fixture(variant):
    with np.load(os.path.join(GOLDEN, "ref_cloud_%s.npz" % variant)) as z:
        return {k: z[k] for k in z.files}


def record(variant, name):
    fx = fixture(variant)
    return {k: fx[name + "." + k] for k in ref_cloud.FIELDS}


@functools.lru_cache(maxsize=None)
def oracle_answer(variant, name):
    return cc.oracle_cloud(orc.OracleMap, scenario(variant, name), record(variant, name))


CASES = [(v, n) for v in ref_cloud.VARIANTS for n in cc.NAMES[v]]
case = pytest.mark.parametrize("variant,name", CASES, ids=["%s-%s" % c for c in CASES])


def test_names_cover_the_scenarios():
    for variant in ref_cloud.VARIANTS:
        assert sorted(set(k.split(".")[0] for k in fixture(variant))) == sorted(cc.NAMES[variant])
        assert os.path.getsize(os.path.join(GOLDEN, "ref_cloud_%s.npz" % variant)) <= 212604
    # every place the issue names has a scenario
    for variant, name in (("third", "resize_rows"), ("zed2", "track_label"), ("zed2", "static_movable"), ("zed2", "static_movable_clipped"),
                          ("zed2", "zero_objects"), ("zed2", "boundary_id"), ("zed2", "depth_edges"), ("zed2", "derived_box"),
                          ("third", "overlap_ab"), ("third", "overlap_ba"), ("zed2", "sky_and_255"), ("third", "no_static"),
                          ("third", "max_objects"), ("third", "noise_flag_off"), ("plain", "exact_axis"), ("plain", "exact_half")):
        assert (variant, name) in CASES


@case
def test_fixture_is_of_this_scenario(variant, name):
    """the hash stored beside the reference's answer is the one of the scenario file today's builder writes"""
    assert np.array_equal(cc.inputs_hash(ref_cloud.script(scenario(variant, name))), fixture(variant)[name + ".inputs"])


@case
def test_harness_reproduces_fixture(variant, name):
    path = ref_cloud.exe(variant)
    if not os.path.exists(path):
        pytest.skip("no reference harness: %s is missing (make -C oracle ref, with the reference at hand)" % path)
    got = ref_cloud.parse(ref_cloud.run(variant, ref_cloud.script(scenario(variant, name))))
    want = record(variant, name)
    for k in ref_cloud.FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), \
            "the harness no longer answers as recorded: " + k


@case
def test_scenario_hits_its_case(variant, name):
    cc.check_hits(scenario(variant, name), record(variant, name))


@case
def test_oracle_matches_reference(variant, name):
    cloud, depth = oracle_answer(variant, name)
    cc.compare(scenario(variant, name), record(variant, name), cloud, depth, "oracle")


def test_variants_are_the_issue_s():
    want = {"zed2": (3, 1, 1, 0.5), "third": (3, 1, 1, 0.3), "plain": (2, 0, 1, 1.0), "static": (0, 0, 0, 1.0)}
    for variant, (setting, boost, consider, rescale) in want.items():
        rec = record(variant, cc.NAMES[variant][0])
        assert rec["variant"].tolist() == [setting, boost, consider, cc.W, cc.H]
        assert rec["camera"][6] == np.float32(rescale)
        assert np.array_equal(rec["camera"][:6], np.array(cc.DESIGN_CAMERA[variant] + cc.DESIGN_DEPTH, np.float32))
        for name in cc.NAMES[variant]:   # one configuration per variant
            for k in ("variant", "camera", "max_movable", "sky", "label_to_instance", "instance_to_label"):
                assert np.array_equal(record(variant, name)[k], rec[k])
        # the library finds a static instance's label by searching the label -> instance table: the same answer as
        # the reference's instance -> label table
        table = rec["label_to_instance"]
        for inst, label in rec["instance_to_label"]:
            assert int(np.flatnonzero(table[:256] == inst)[0]) == label
        assert table[255] == table[256] == 0    # static-mask value 255 is label 256; the library's table ends at 255


def test_float_back_projection_fails_the_position_rule():
    """the cap is not vacuous: the same formula in float32 is caught in every random scenario with a tilted pose"""
    for variant, name in (("third", "resize_rows"), ("zed2", "boundary_id"), ("plain", "plain_boundary")):
        sc, rec = scenario(variant, name), record(variant, name)
        pos = cc.backproject(rec["depth"], rec["camera"], sc["pose"], np.float32).reshape(-1, 3)[rec["pixel"]]
        worst, share = cc.position_report(rec["pos"], pos)
        assert share > 100 * cc.AMBIGUOUS_CAP, (variant, name, worst, share)
        with pytest.raises(AssertionError):
            cc.check_positions(rec["pos"], pos, False, "float32")
        # while the double restatement passes it, as the oracle does
        pos = cc.backproject(rec["depth"], rec["camera"], sc["pose"], np.float64).reshape(-1, 3)[rec["pixel"]].astype(np.float32)
        cc.check_positions(rec["pos"], pos, False, "float64")


def test_exact_scenarios_do_not_depend_on_the_formula():
    """in an exact scenario even the float32 restatement gives the reference's bits or fails by whole floats, never by
    the order of a sum: the double one, with another association of the three-term sums, gives the same bits"""
    for name in ("exact_axis", "exact_half"):
        sc, rec = scenario("plain", name), record("plain", name)
        d = rec["depth"].astype(np.float64)
        j, i = np.meshgrid(np.arange(cc.W, dtype=np.float64), np.arange(cc.H, dtype=np.float64))
        fx, fy, cx, cy = (float(v) for v in rec["camera"][:4])
        x, y, z = (j - cx) / fx * d, (i - cy) / fy * d, d
        r = cc.rotation(sc["pose"][3:])
        pos = np.stack([sc["pose"][a] + (r[a, 2] * z + (r[a, 1] * y + r[a, 0] * x)) for a in range(3)], axis=-1).reshape(-1, 3)[rec["pixel"]]
        assert np.array_equal(pos.astype(np.float32).view(np.uint32), rec["pos"].view(np.uint32)), name


def test_box_rule_is_what_the_clipping_implies():
    """the Python restatement of :180-199 (max starts at DBL_MIN, +- 1 m), which the tests hand to the library as
    object_bbox, predicts the recorded clipping: the box of the LAST entry with the pixel's track id, zeros for an id
    without an entry"""
    total = 0
    for variant in ("zed2", "third"):
        for name in cc.NAMES[variant]:
            sc, rec = scenario(variant, name), record(variant, name)
            ids = cc.merged_ids(sc, rec).reshape(-1)[rec["pixel"]]
            pos = cc.backproject(rec["depth"], rec["camera"], sc["pose"]).reshape(-1, 3)[rec["pixel"]]
            boxes = {}
            for t, _, kpts, _ in sc["dst"]["objects"]:
                boxes[t] = cc.box_rule(kpts)
            b = np.array([boxes.get(int(t), np.zeros(6)) for t in ids]).reshape(-1, 3, 2)
            outside = ((pos < b[:, :, 0]) | (pos > b[:, :, 1])).any(axis=1) & (ids < int(rec["max_movable"][0]))
            near = (np.abs(pos[:, :, None] - b).min(axis=(1, 2)) < 1e-9)     # on a face: the double formulas may disagree
            assert np.array_equal(outside[~near], rec["clipped"][~near] > 0), (variant, name)
            total += int(outside.sum())
    assert total > 2000
    b = cc.box_rule(np.array([[-3.0, -2.0, -2.5], [-2.0, -1.5, -1.0]]))
    assert b.tolist() == [-4.0, 1.0, -3.0, 1.0, -3.5, 1.0]
    e = cc.box_rule(np.zeros((0, 3)))
    assert np.all(e[0::2] == np.finfo(np.float64).max) and np.all(e[1::2] == 1.0)


def test_adapter_header_restates_the_box_rule():
    """include/semantic_dsp_map.h derives the boxes it hands to sdm_update_raw_ex; its text must start the max at
    numeric_limits<double>::min() and add the 1 m margin, as box_rule() does"""
    with open(os.path.join(ROOT, "include", "semantic_dsp_map.h")) as f:
        text = f.read()
    body = text[text.index("pointcloud_tools.h:174-196"):]
    body = body[:body.index("++k_obj")]
    assert len(re.findall(r"double lo\[3\] = \{std::numeric_limits<double>::max\(\)", body)) == 1
    assert len(re.findall(r"double hi\[3\] = \{std::numeric_limits<double>::min\(\), std::numeric_limits<double>::min\(\), std::numeric_limits<double>::min\(\)\}", body)) == 1
    assert "const double margin = 1.0;" in body and "lo[a] - margin" in body and "hi[a] + margin" in body


def test_adapter_table_against_the_record():
    """synth.LABEL_TO_STATIC_INSTANCE (the table the adapter builds from cfg/object_info.csv) and the record: the
    project's table follows the csv's label ids, the record the defaults compiled into utils/data_base.h, so the two
    are compared by NAME through the static instance ids, which both take from the same list; where a label has no
    static instance the adapter's table holds 65535 and the reference's default insertion gives 0 - the caller's
    documented choice."""
    rec = record("zed2", "track_label")
    table = rec["label_to_instance"]
    to_label = {int(i): int(l) for i, l in rec["instance_to_label"]}
    assert set(to_label) == set(range(65524, 65536))
    assert sorted(int(v) for v in table if v) == sorted(to_label)           # every static instance once, everything else 0
    # the adapter's compiled-in defaults (defaultLabelTables): names, label ids, instance 65535 - i for the first twelve
    with open(os.path.join(ROOT, "include", "semantic_dsp_map.h")) as f:
        text = f.read()
    body = text[text.index("void defaultLabelTables()"):]
    names = re.findall(r'"(\w+)"', body[body.index("names[] = {"):body.index("};")])
    ids = [int(v) for v in re.findall(r"\d+", body[body.index("ids[] = {"):].split("}")[0].split("{")[1])]
    assert len(names) == len(ids) == 15 and "static_instance_to_label_[65535 - i] = ids[i]" in body and "max_movable_track_ = 65523;" in body
    for i in range(12):
        assert table[ids[i]] == 65535 - i and to_label[65535 - i] == ids[i], names[i]
    for i in range(12, 15):                                                  # Truck, Car, Person: a name, no static instance
        assert table[ids[i]] == 0
    assert int(rec["max_movable"][0]) == 65523
    movable = {"Truck": 13, "Car": 14, "Person": 15}
    for sc_name in ("track_label", "static_movable"):
        sc, r = scenario("zed2", sc_name), record("zed2", sc_name)
        for e, label in zip(sc["entries"], r["entry_labels"]):
            assert label == (-1 if e["label"] == "static" else movable[e["label"]]) and (e["label"] == "static" or ids[names.index(e["label"])] == label)
    # the synthetic scenes' table: the csv's, which shares label ids 3 ... 12 with the defaults
    ours = synth.LABEL_TO_STATIC_INSTANCE
    assert ours.shape == (256,) and not (ours == 0).any()
    for l in range(256):
        if l == 0 or 3 <= l <= 12:
            assert ours[l] == table[l], l                                    # every named static label both lists hold
        elif l == 13:
            assert ours[l] == 65523 and synth.MAX_MOVABLE_TRACK == 65522     # the csv's thirteenth static class
        else:
            assert ours[l] == 65535 and (table[l] == 0 or l == 2)            # no static instance: 65535 here, 0 there (2: Terrain, not in the csv)
