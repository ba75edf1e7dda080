"""The two restatements of the world objects (tests/world_objects_ref.py) against each other on every case of
tests/world_objects_cases.py, the cases' closed forms, and three checks that the cases discriminate: a model whose
3 x 3 x 3 growth is masked stage by stage, one without the column masks of the x shifts and one without the seam pass each
get a case wrong that the full model gets right.  No GPU."""
import numpy as np
import pytest

from tests import world_objects_cases as oc
from tests import world_objects_ref as wor

SIZE = np.float32(oc.CFG["voxel_size"])
CASES = oc.crafted()


def models(c, kw, **fault):
    return wor.BrickModel(c["hdr"], c["cells"], SIZE, oc.MM, **kw, **fault)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_models_agree_on_the_crafted_cases(name):
    c = CASES[name]
    for k, (kw, _) in enumerate(c["builds"]):
        a = models(c, kw)
        b = wor.CellModel(c["hdr"], c["cells"], SIZE, oc.MM, **kw)
        diff = wor.difference(wor.answer(a), wor.answer(b))
        assert diff is None, (name, kw, diff)
        oc.check_closed_forms(name, c, k, a)
        assert (a.table["pad0"] == 0).all() and (a.table["pad1"] == 0).all()
        assert int(a.label_cells.sum()) == a.info["n_cells"] and int(a.label_objects.sum()) == a.info["n_objects_total"]


def test_the_two_models_agree_on_the_random_archive():
    hdr, cells = oc.random_archive()
    seen = set()
    for kw in oc.random_variants():
        a = wor.BrickModel(hdr, cells, SIZE, oc.MM, **kw)
        b = wor.CellModel(hdr, cells, SIZE, oc.MM, **kw)
        diff = wor.difference(wor.answer(a), wor.answer(b))
        assert diff is None, (kw, diff)
        assert a.info["n_cells"] > 1000 and a.info["n_objects_total"] > a.info["n_objects"] - (kw.get("min_cells", 1) == 1) >= 0
        seen.add((int(a.info["flags"]), int(a.info["min_cells"])))
    assert len(seen) == 17


def test_a_query_of_the_model_finds_every_cell_and_nothing_else():
    c = CASES["filters"]
    a = models(c, dict(min_cells=3))
    res = a.query(cells=a.cells)
    assert np.array_equal(res["index"], np.arange(len(a.cells))) and np.array_equal(res["object"], a.object)
    assert (a.object == wor.WORLD_OBJECT_UNLISTED).sum() == 2
    res = a.query(cells=[(15, 15, 15), (0, 0, 0), (8 * 40000, 0, 0)])
    assert (res["object"] == wor.WORLD_OBJECT_NONE).all() and (res["index"] == wor.WORLD_OBJECT_NONE).all()
    pts = (a.cells[:3].astype(np.float32) + np.float32(0.5)) * SIZE
    assert np.array_equal(a.query(xyz=pts, voxel_size=SIZE)["index"], [0, 1, 2])
    bad = a.query(xyz=[(np.nan, 0, 0), (np.inf, 0, 0), (3e7, 0, 0)], voxel_size=SIZE)
    assert (bad["object"] == wor.WORLD_OBJECT_NONE).all() and (bad["cell"] == 0).all()


# ---- the cases discriminate
def test_a_stage_masked_growth_misses_the_diagonal_pair():
    wrong = 0
    for name, c in CASES.items():
        if not name.startswith("pair "):
            continue
        right = models(c, {})
        assert right.label_objects[1] == 1, name
        wrong += models(c, {}, separable=True).label_objects[1] != 1 if name.endswith("inside") else 0
    assert wrong == 8          # every pair inside a brick, whatever lies between: 2 kinds x 4 fillers


def test_a_model_without_the_column_masks_joins_across_the_x_wrap():
    c = CASES["x wrap"]
    for kw, want in c["builds"]:
        assert models(c, kw).info["n_objects_total"] == want["total"] == 4
        assert models(c, kw, wrap_mask=False).info["n_objects_total"] < 4


def test_a_model_without_the_seam_pass_misses_every_seam_variant():
    names = [n for n in CASES if n.startswith("pair ") and not n.endswith("inside")] + ["seam face", "bridge x", "serpentine tube", "plate"]
    assert len(names) == 20 + 4
    for name in names:
        c = CASES[name]
        kw = dict(face_connected=True) if name == "seam face" else {}
        right, wrong = models(c, kw), models(c, kw, seams=False)
        if name == "bridge x":          # (its three cells never join: the seam pass must not change it)
            assert right.info["n_objects_total"] == wrong.info["n_objects_total"] == 3
        else:
            assert wrong.info["n_objects_total"] > right.info["n_objects_total"], name
