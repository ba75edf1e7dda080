"""tests/world_changes_ref.py's two restatements of the world changes (include/sdm.h) against each other, without a GPU, on
every crafted pair of tests/world_changes_cases.py and on the random pair, under every build each case lists; the closed
forms the cases state; and what must hold of any answer: the counters sum to the known cells of both sides, the listed
cells are a subset of the three change classes, the regions' cells sum to the list.  The block side reading occ == 2, which
no crafted map state produces, is covered here."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import shape_cases as sc
from tests import world_changes_cases as cc
from tests import world_changes_ref as wcr

CASES = cc.crafted()
RANDOM = cc.random_pair()
CHANGES = ("n_appeared", "n_vanished", "n_relabelled")


def models(c, kw, snap=None):
    cfg = sc.config(c["shape"])
    args = (cc.block_words(c) if snap is None else snap, c["steps"], sc.GTS, c["hdr"], c["cells"], 1, np.float32(cfg["voxel_size"]),
            cfg["max_movable_track"])
    return wcr.BrickModel(*args, **kw), wcr.CellModel(*args, **kw)


def check_invariants(c, ref, kw):
    info = ref.info
    same_new = sum(int(info[n]) for n in CHANGES + ("n_same_occupied", "n_same_free"))
    assert int(info["n_known_now"]) == same_new + int(info["n_new_occupied"]) + int(info["n_new_free"])
    assert int(info["n_known_before"]) == same_new + int(info["n_remembered"])
    assert int(info["n_outside"]) == 512 * int(info["n_candidates"]) - c["occ"].size
    assert int(info["n_known_now"]) <= c["occ"].size
    assert set(ref.cls.tolist()) <= set(binding.ALL_CHANGE_CLASSES) and len(ref.cells) == info["n_cells"]
    for k, name in zip(binding.ALL_CHANGE_CLASSES, CHANGES):
        assert int((ref.cls == k).sum()) <= int(info[name])
    if set(kw.get("classes", binding.ALL_CHANGE_CLASSES)) == set(binding.ALL_CHANGE_CLASSES) and "labels" not in kw:
        assert len(ref.cells) == sum(int(info[n]) for n in CHANGES)
    assert int(ref.appeared.sum() + ref.vanished.sum() + ref.relabelled.sum()) == len(ref.cells)
    if kw.get("min_cells", 1) <= 1:
        assert int(ref.table["n_cells"].sum()) == len(ref.cells) and (ref.region != binding.WORLD_CHANGE_UNLISTED).all()
    else:
        small = ref.region == binding.WORLD_CHANGE_UNLISTED
        assert int(ref.table["n_cells"].sum()) == int((~small).sum()) and (ref.table["n_cells"] >= kw["min_cells"]).all()
    if kw.get("by_label"):
        assert not ref.table["mixed"].any()
    assert np.array_equal(ref.table["first_index"], np.sort(ref.table["first_index"]))


def check_expect(ref, want):
    for name, v in want.items():
        if name.endswith("_min"):
            assert int(ref.info[name[:-4]]) >= v, (name, ref.info)
        else:
            assert int(ref.info[name]) == v, (name, int(ref.info[name]), v)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_restatements_agree_on_the_crafted_pairs(name):
    c = CASES[name]
    for kw, want in c["builds"]:
        a, b = models(c, kw)
        diff = wcr.difference(wcr.answer(a), wcr.answer(b))
        assert diff is None, (name, kw, diff)
        check_expect(a, want)
        check_invariants(c, a, kw)


def test_the_two_restatements_agree_on_the_random_pair():
    seen = set()
    for kw, _ in RANDOM["builds"]:
        a, b = models(RANDOM, kw)
        diff = wcr.difference(wcr.answer(a), wcr.answer(b))
        assert diff is None, (kw, diff)
        check_invariants(RANDOM, a, kw)
        assert a.info["n_cells"] > 200 and a.info["n_regions_total"] > 20
        seen.add(int(a.info["flags"]))
    assert len(seen) == 32 - 14           # the sixteen flag sets, and OLDER on two of them


def test_every_cell_of_the_class_table_counts():
    for name in ("class table at 0", "class table at 7", "class table"):
        a, _ = models(CASES[name], {})
        for counter in binding.WORLD_CHANGES_COUNTERS:
            assert a.info[counter] > 0, (name, counter)
        assert a.info["n_candidates"] == {"class table at 0": 1, "class table": 2, "class table at 7": 8}[name]
    c = CASES["class table"]
    base = {n: int(a.info[n]) for n in binding.WORLD_CHANGES_COUNTERS}
    obs, _ = models(c, dict(observed_only=True))          # the guessed archived cell no longer counts as the same
    assert obs.info["n_same_occupied"] == base["n_same_occupied"] - 1 and obs.info["n_new_occupied"] == base["n_new_occupied"] + 1
    stat, _ = models(c, dict(static_only=True))           # the movable tracks read unknown on either side
    assert stat.info["n_vanished"] == base["n_vanished"] - 1 and stat.info["n_new_free"] == base["n_new_free"] + 1
    assert stat.info["n_appeared"] == base["n_appeared"] - 1 and stat.info["n_remembered"] == base["n_remembered"] + 1


def test_a_block_that_guesses_reads_unknown_when_only_the_observed_count():
    c = CASES["class table"]
    snap = cc.block_words(c)
    guessed = (snap >> 24) == 1
    snap[guessed] = (snap[guessed] & 0x00FFFFFF) | np.uint32(2 << 24)
    for kw in ({}, dict(observed_only=True), dict(observed_only=True, static_only=True, by_label=True)):
        a, b = models(c, kw, snap)
        assert wcr.difference(wcr.answer(a), wcr.answer(b)) is None, kw
        if kw.get("observed_only"):
            assert a.info["n_appeared"] == a.info["n_relabelled"] == a.info["n_same_occupied"] == a.info["n_new_occupied"] == 0
        else:
            plain, _ = models(c, kw)
            assert a.info.tobytes() == plain.info.tobytes() and a.table.tobytes() == plain.table.tobytes()


def test_the_bridge_joins_over_another_label_only_without_by_label():
    c = CASES["vanished shapes"]
    plain, _ = models(c, {})
    by_label, _ = models(c, dict(by_label=True))
    q = plain.query(cells=(np.array([[2, 0, 60], [3, 0, 60], [4, 0, 60]]) + cc.box_of(sc.config("C"), c["steps"])[0]))
    assert len(set(q["region"].tolist())) == 1 and plain.table["mixed"][q["region"][0]] == 1 and plain.table["n_cells"][q["region"][0]] == 3
    q = by_label.query(cells=q["cell"])
    assert len(set(q["region"].tolist())) == 3
    q = plain.query(cells=(np.array([[2, 3, 50], [3, 3, 50], [4, 3, 50]]) + cc.box_of(sc.config("C"), c["steps"])[0]))
    assert len(set(q["region"].tolist())) == 3 and q["cls"].tolist() == [2, 1, 2]
