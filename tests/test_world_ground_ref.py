"""The two restatements of the world ground layer (tests/world_ground_ref.py) against each other on every case of
tests/world_ground_cases.py, and against the values the cases carry, worked out by hand.  No GPU."""
import numpy as np
import pytest

from tests import world_ground_cases as gc
from tests import world_ground_ref as wgr

SIZE = np.float32(gc.CFG["voxel_size"])
CASES = gc.crafted()


def both(hdr, cells, **kw):
    a = wgr.ColumnModel(hdr, cells, max_movable=gc.MM, stamp=3, **kw)
    b = wgr.DenseModel(hdr, cells, max_movable=gc.MM, stamp=3, **kw)
    diff = wgr.difference(wgr.answer(a), wgr.answer(b))
    assert diff is None, diff
    return a


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_archives(name):
    c = CASES[name]
    m = both(c["hdr"], c["cells"], **c["kw"])
    c["expect"](m)
    assert m.info["n_ground"] + m.info["n_obstacle"] + m.info["n_none"] == 64 * m.info["n_tiles"]
    assert (m.cells["headroom"][(m.cells["cls"] & 3) == 1] >= min(c["kw"]["clearance"], 255)).all()


def test_the_random_archive_under_every_option():
    hdr, cells = gc.random_world()
    seen, lethal = set(), set()
    for kw in gc.random_variants():
        m = both(hdr, cells, **kw)
        seen.add((int(m.info["options"]["flags"]), int(m.info["options"]["radius"]), int(m.info["options"]["up_axis"])))
        lethal.add(int(m.info["n_lethal"]))
        assert m.info["n_ground"] > 0 and m.info["n_tiles"] > 0
    assert len(seen) == 16 * 2 * 3 + 1 and len(lethal) > 8


def test_queries_on_the_corner():
    c = gc.corner_case()
    m = both(c["hdr"], c["cells"], **c["kw"])
    lv = {(i, j): int(gc.column(m, i, j)[0]["level"]) for i in (-8, -1, 0, 7) for j in (-8, -1, 0, 7)}
    assert all(v == (3 if i >= 0 and j >= 0 else 0) for (i, j), v in lv.items()), lv
    assert gc.column(m, 0, 3)[0]["cls"] == 1 | 4 | 8 and gc.column(m, -1, 3)[0]["cls"] == 1 and gc.column(m, -2, 1)[0]["cls"] == 2 | 8
    q = m.query([(0, 0, 9), (-1, 0, 0), (-2, 1, 5), (8, 0, 0), (1 << 20, 0, 0)], SIZE)
    assert q["status"].tolist() == [0, 0, 0, 3, 3] and q["col"].tolist() == [[0, 0], [-1, 0], [-2, 1], [8, 0], [0, 0]]
    assert q["above"].tolist() == [6, 0, wgr.INT32_MIN, wgr.INT32_MIN, wgr.INT32_MIN] and q["surface"].tolist() == [4.0, 1.0, 0.0, 0.0, 0.0]
    assert q["d2"].tolist() == [0, 1, 0, 0xFFFFFFFF, 0xFFFFFFFF] and q["dist"].tolist() == [0.0, 1.0, 0.0, -1.0, -1.0]
    f = m.footprints(gc.footprint_set(), SIZE)
    # (0, 0) +- (2.6, 1.2): the centres -2.5 .. 2.5 by -0.5 .. 0.5 - six by two columns, of which (0, 0), (1, 0), (2, 0) lie on
    # the higher tile's marked rim
    assert tuple(f[0])[:5] == (12, 3, 0, 12, 0) and f[0]["first_lethal"].tolist() == [0, 0] and (f[0]["level_min"], f[0]["level_max"]) == (0, 3)
    assert f[0]["min_d2"] == 0
    # (7, 0) +- (3, 1): centres 4.5 .. 9.5 by -0.5 .. 0.5: eight columns of tiles, four of none
    assert (f[3]["n_cols"], f[3]["n_absent"]) == (8, 4)
    for k in (4, 6, 7, 8, 10):   # too large, non-finite, no heading, beyond the range
        assert f[k].tobytes() == f[6].tobytes() and f[k]["n_cols"] == f[k]["n_absent"] == 0 and f[k]["min_d2"] == 0xFFFFFFFF
    assert (f[5]["n_cols"], f[5]["n_absent"]) == (256, 80 * 48 - 256)
    assert (f[9]["n_cols"], f[9]["n_absent"], f[9]["min_d2"]) == (0, 20, 0xFFFFFFFF)
    assert (f[11]["n_cols"], f[11]["n_ground"], f[11]["level_min"]) == (1, 1, 3) and f[12]["n_cols"] == 0


def test_what_a_model_without_the_seam_rules_gets_wrong():
    """the cases tell such models apart: the word's wrap, the sign's mapping"""
    c = CASES["x wrap"]
    m = wgr.ColumnModel(c["hdr"], c["cells"], max_movable=gc.MM, **c["kw"])
    assert gc.column(m, 0, 3)[1] == 50          # a row that wrapped inside the word would give 1
    up, down = CASES["orientation 2 +1 at -1"], CASES["orientation 2 -1 at -1"]
    a = wgr.ColumnModel(up["hdr"], up["cells"], max_movable=gc.MM, **up["kw"])
    b = wgr.ColumnModel(down["hdr"], down["cells"], max_movable=gc.MM, **down["kw"])
    assert a.cells["level"][0, 0] == 3 and b.cells["level"][0, 0] == 4 and up["kw"]["h_lo"] == -8 and down["kw"]["h_lo"] == 0
