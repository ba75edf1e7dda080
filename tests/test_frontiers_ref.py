"""tests/frontiers_ref.py (the restatement the GPU tests compare with) against a brute-force flood fill in pure Python,
and against scipy.ndimage.label where SciPy is installed; the cluster struct's size as ctypes and NumPy see it against
the header's."""
import ctypes as C
import os
import re
from collections import deque

import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import frontiers_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [(4, 8, 4), (8, 4, 16)]   # [NZ, NY, NX]
ORIGIN = np.array([-1.5, 0.25, 3.0], np.float32)
SIZE = 0.3


def random_block(shape, seed):
    return np.random.default_rng(seed).choice(np.array([0, -1, 1], np.int8), size=shape, p=[0.5, 0.3, 0.2])


def brute_force(occ, face_connected, min_cells):
    """frontier cells by the definition, clusters by breadth-first search -> [(first_cell, cells, faces per cell)]"""
    NZ, NY, NX = occ.shape
    six = [(0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)]
    steps = six if face_connected else [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    faces = {}
    for z in range(NZ):
        for y in range(NY):
            for x in range(NX):
                if occ[z, y, x] != 0:
                    continue
                n = sum(1 for dz, dy, dx in six
                        if 0 <= z + dz < NZ and 0 <= y + dy < NY and 0 <= x + dx < NX and occ[z + dz, y + dy, x + dx] == -1)
                if n:
                    faces[(z, y, x)] = n
    seen, clusters = set(), []
    for start in sorted(faces):
        if start in seen:
            continue
        seen.add(start)
        todo, cells = deque([start]), []
        while todo:
            z, y, x = todo.popleft()
            cells.append((z, y, x))
            for dz, dy, dx in steps:
                q = (z + dz, y + dy, x + dx)
                if q in faces and q not in seen:
                    seen.add(q)
                    todo.append(q)
        clusters.append(sorted(cells))
    word = lambda c: c[2] + NX * (c[1] + NY * c[0])  # noqa: E731
    return faces, [c for c in clusters if len(c) >= max(min_cells, 1)], word


@pytest.mark.parametrize("shape", BLOCKS)
@pytest.mark.parametrize("face_connected", [False, True])
@pytest.mark.parametrize("min_cells", [0, 1, 2, 3, 6])
def test_against_flood_fill(shape, face_connected, min_cells):
    for seed in range(4):
        occ = random_block(shape, 10 * seed + shape[0])
        ref = fr.frontiers_of_block(occ, ORIGIN, SIZE, face_connected, min_cells)
        faces, clusters, word = brute_force(occ, face_connected, min_cells)
        assert ref["cell"].tolist() == sorted(word(c) for c in faces)
        assert ref["unknown_faces"].tolist() == [faces[c] for c in sorted(faces)]
        t = ref["table"]
        assert len(t) == len(clusters) and (np.diff(t["first_cell"].astype(np.int64)) > 0).all()
        position = {int(w): i for i, w in enumerate(ref["cell"])}
        member = np.full(len(ref["cell"]), fr.FRONTIER_NO_CLUSTER, np.uint32)
        size = np.float32(SIZE)
        for j, (e, cells) in enumerate(zip(t, clusters)):
            words = [word(c) for c in cells]
            member[[position[w] for w in words]] = j
            assert e["first_cell"] == words[0] and e["first_index"] == position[words[0]] and e["n_cells"] == len(cells)
            assert e["n_unknown_faces"] == sum(faces[c] for c in cells)
            for a in range(3):
                v = [c[2 - a] for c in cells]
                assert e["cell_min"][a] == min(v) and e["cell_max"][a] == max(v) and e["cell_sum"][a] == sum(v)
                assert e["box_min"][a] == ORIGIN[a] + np.float32(min(v)) * size
                assert e["box_max"][a] == ORIGIN[a] + np.float32(max(v) + 1) * size
                assert e["centroid"][a] == np.float32(np.float64(ORIGIN[a]) + (np.float64(sum(v)) / np.float64(len(v)) + 0.5) * np.float64(size))
            assert e["pad0"] == 0 and e["pad1"] == 0
        assert np.array_equal(ref["cluster"], member)
        if min_cells <= 1:
            assert len(t) >= 1 and (member != fr.FRONTIER_NO_CLUSTER).all()


@pytest.mark.parametrize("shape", BLOCKS + [(16, 16, 16)])
@pytest.mark.parametrize("face_connected", [False, True])
def test_against_scipy_label(shape, face_connected):
    ndimage = pytest.importorskip("scipy.ndimage")
    occ = random_block(shape, 5)
    mask, _ = fr.frontier_mask(occ)
    structure = ndimage.generate_binary_structure(3, 1 if face_connected else 3)
    lab, n = ndimage.label(mask, structure=structure)
    flat = lab.ravel()
    cells = np.flatnonzero(flat)
    first = np.full(n + 1, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, flat[cells], cells)            # labels normalised to first_cell
    ref = fr.frontiers_of_block(occ, ORIGIN, SIZE, face_connected, 1)
    assert np.array_equal(ref["cell"], cells) and len(ref["table"]) == n
    assert np.array_equal(ref["table"]["first_cell"][ref["cluster"]], first[flat[cells]])


def test_long_snake_labels_in_few_rounds():
    """one 6-connected component that winds through every row of a 64 x 64 plane"""
    occ = np.full((64, 2, 64), -1, np.int8)
    for z in range(64):
        if z % 2 == 0:
            occ[z, 0, :] = 0
        else:
            occ[z, 0, 63 if z % 4 == 1 else 0] = 0
    ref = fr.frontiers_of_block(occ, ORIGIN, SIZE, True, 1)
    assert len(ref["table"]) == 1 and ref["table"]["n_cells"][0] == 32 * 64 + 32 and ref["table"]["first_cell"][0] == 0


def test_struct_size_matches_the_header():
    text = open(os.path.join(ROOT, "semantic_dsp_map_amd", "csrc", "frontiers.hip")).read()
    size = int(re.search(r"static_assert\(sizeof\(sdm_frontier_cluster\) == (\d+)", text).group(1))
    header = open(os.path.join(ROOT, "include", "sdm.h")).read()
    per_cell = int(re.search(r"#define SDM_FRONTIERS_BYTES_PER_CELL (\d+)", header).group(1))

    class Cluster(C.Structure):
        _fields_ = [("first_cell", C.c_uint32), ("n_cells", C.c_uint32), ("n_unknown_faces", C.c_uint32), ("first_index", C.c_uint32),
                    ("cell_min", C.c_uint16 * 3), ("cell_max", C.c_uint16 * 3), ("pad0", C.c_uint32), ("cell_sum", C.c_uint64 * 3),
                    ("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("centroid", C.c_float * 3), ("pad1", C.c_uint32)]
    assert C.sizeof(Cluster) == size == binding.FRONTIER_CLUSTER.itemsize and size % 8 == 0
    for name, _ in Cluster._fields_:
        assert getattr(Cluster, name).offset == binding.FRONTIER_CLUSTER.fields[name][1], name
    assert per_cell > size
