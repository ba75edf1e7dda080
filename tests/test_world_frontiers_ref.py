"""The two restatements of the world frontiers (tests/world_frontiers_ref.py) against each other on every case of
tests/world_frontiers_cases.py - cells, unknown_faces, cluster indices, table and info -, against what is known in closed
form, and the two discrimination checks: a model without the wrap mask of the x shifts differs on the x-wrap case, and
brick-local labelling alone, the seam pass left out, gives more clusters on every seam variant.  No GPU."""
import numpy as np
import pytest

from tests import world_frontiers_cases as fc
from tests import world_frontiers_ref as wfr

CASES = fc.crafted()
SIZE = np.float32(fc.CFG["voxel_size"])


def both(c, **more):
    kw = dict(c["kw"], **more)
    a = wfr.BrickModel(c["hdr"], c["cells"], SIZE, **kw)
    b = wfr.CellModel(c["hdr"], c["cells"], SIZE, **kw)
    diff = wfr.difference(wfr.answer(a), wfr.answer(b))
    assert diff is None, diff
    # the list ascends in (brick rank, cell word), the table in first_index, and a cluster's first cell is its smallest
    rank = {tuple(q): r for r, q in enumerate(a.coords.tolist())}
    key = [(rank[tuple((c >> 3).tolist())], int((c[0] & 7) | (c[1] & 7) << 3 | (c[2] & 7) << 6)) for c in a.cells.astype(np.int64)]
    assert key == sorted(set(key))
    assert (np.diff(a.table["first_index"].astype(np.int64)) > 0).all() and (a.table["pad0"] == 0).all()
    assert int(a.table["n_cells"].sum()) == int((a.cluster != 0xFFFFFFFF).sum()) and ((a.faces >= 1) & (a.faces <= 6)).all()
    return a


def check_closed_forms(name, a):
    """what the issue states about a case; the GPU test asserts the same of the library"""
    t, info = a.table, a.info
    if name in ("one free", "one free at -1"):
        lo = 0 if name == "one free" else -8
        assert info["n_cells"] == 296 == t[0]["n_cells"] and len(t) == 1 and info["n_unknown_faces"] == 384 == info["n_absent_faces"]
        on_border = ((a.cells == lo) | (a.cells == lo + 7)).sum(axis=1)
        assert np.array_equal(a.faces, on_border) and sorted(np.bincount(a.faces).tolist()) == [0, 8, 72, 216]
        assert t[0]["cell_min"].tolist() == [lo] * 3 and t[0]["cell_max"].tolist() == [lo + 7] * 3
        assert t[0]["cell_sum"].tolist() == [296 * (2 * lo + 7) // 2] * 3 and (lo == 0 or t[0]["cell_sum"][0] < 0)
        assert t[0]["centroid"].tolist() == [np.float32((lo + 4) * np.float64(SIZE))] * 3
    elif name == "one free inside" or name == "x wrap":
        assert info["n_cells"] == 0 and len(t) == 0 and info["n_bricks"] == 1
    elif name.startswith("hole"):
        assert info["n_cells"] == 6 and (a.faces == 1).all() and info["n_absent_faces"] == 0
        assert len(t) == (6 if name == "hole face" else 1)
    elif name.startswith("seams"):
        kind, face = name.split()[1], name.endswith(" face")
        assert info["n_cells"] == 2 and len(t) == (1 if kind == "face" or not face else 2) and info["n_bricks"] == 8
        assert sorted(a.cells.tolist()) == sorted(list(p) for p in CASES[name]["pair"])
    elif name == "absent neighbour":
        assert info["n_cells"] == 16 * 64 - 14 * 36 and info["n_absent_faces"] == 2 * (16 * 8 + 16 * 8 + 64) == info["n_unknown_faces"]
        inner = ((a.cells[:, 0] == 7) | (a.cells[:, 0] == 8))
        assert (a.faces[inner] == ((a.cells[inner, 1:] == 0) | (a.cells[inner, 1:] == 7)).sum(axis=1)).all() and len(t) == 1
    elif name == "box":
        assert info["n_bricks"] == 1 and info["n_cells"] == 512 - 7 * 36 and info["n_absent_faces"] == 5 * 64 and len(t) == 1
        assert t[0]["cell_max"].tolist() == [7, 7, 7] and not ((a.cells[:, 0] == 7) & (a.faces > 2)).any()
    elif name.startswith("serpentine"):
        assert info["n_bricks"] == 30 and info["n_absent_faces"] == 0
        if name == "serpentine":
            assert len(t) == 1 and t[0]["first_index"] == 0 and t[0]["first_cell"].tolist() == a.cells[0].tolist() and t[0]["n_cells"] == info["n_cells"] > 1500
    elif name == "plate":
        assert info["n_bricks"] == 2116 and info["n_cells"] == 4 * 368 - 4 and info["n_unknown_faces"] == 4 * 368 == info["n_absent_faces"] and len(t) == 1
    elif name == "int16 edge":
        assert info["n_bricks"] == 12 and len(t) == 12 and (t["n_cells"] == 296).all() and info["n_absent_faces"] == 12 * 384
    else:
        raise AssertionError(name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_restatements_agree(name):
    check_closed_forms(name, both(CASES[name]))


@pytest.mark.parametrize("kw", fc.random_variants(), ids=lambda kw: " ".join("%s=%s" % (k, v) for k, v in sorted(kw.items())))
def test_the_two_restatements_agree_on_the_random_archive(kw):
    hdr, cells = fc.random_archive()
    a = both(dict(hdr=hdr, cells=cells, kw=kw))
    assert a.info["n_cells"] > 500 and a.info["n_clusters_total"] >= a.info["n_clusters"] >= 1
    if kw["min_cells"] > 1:
        assert (a.table["n_cells"] >= kw["min_cells"]).all()
        if kw["face_connected"]:   # (26-connected the random archive's frontier is all but one cluster)
            assert a.info["n_clusters_total"] > a.info["n_clusters"] and (a.cluster == 0xFFFFFFFF).any()
    if kw["box"]:
        assert 0 < a.info["n_bricks"] < len(hdr)
    if not kw["inside_bricks"]:
        assert a.info["n_absent_faces"] > 0


def test_empty_fields():
    c = CASES["one free"]
    for box in (((100, 100, 100), (101, 101, 101)), ((0, 0, 0), (0, -1, 0))):
        a = both(c, box=box)
        assert a.info["n_bricks"] == 0 and a.info["n_cells"] == 0 and len(a.table) == 0
    a = both(dict(hdr=c["hdr"][:0], cells=c["cells"][:0], kw={}))
    assert a.info["n_bricks"] == 0 and a.info["n_cells"] == 0


def test_a_model_without_the_wrap_mask_differs_on_the_x_wrap_case():
    c = CASES["x wrap"]
    wrong = wfr.BrickModel(c["hdr"], c["cells"], SIZE, wrap_mask=False, **c["kw"])
    assert sorted(wrong.cells.tolist()) == [[0, 6, 5], [7, 2, 2]] and wfr.CellModel(c["hdr"], c["cells"], SIZE, **c["kw"]).info["n_cells"] == 0


@pytest.mark.parametrize("kind", ["face", "edge", "corner"])
def test_brick_local_labelling_alone_gives_more_clusters(kind):
    c = CASES["seams " + kind]
    whole, local = wfr.BrickModel(c["hdr"], c["cells"], SIZE, **c["kw"]), wfr.BrickModel(c["hdr"], c["cells"], SIZE, seams=False, **c["kw"])
    assert len(whole.table) == 1 and len(local.table) == 2 and np.array_equal(whole.cells, local.cells)
    s = CASES["serpentine"]
    assert len(wfr.BrickModel(s["hdr"], s["cells"], SIZE, seams=False, **s["kw"]).table) >= 30 if kind == "face" else True
