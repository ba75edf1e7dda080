"""tests/world_mesh_ref.py's two restatements of the world mesh against each other on every case of
tests/world_mesh_cases.py, against the cases' closed forms, and against checks that share no code with them: the normals,
the closed mesh, the divergence theorem in integers, the tiling of disjoint boxes, and tests/mesh_ref.py - the block's
restatement, which knows nothing of bricks - on a dense grid.  No GPU."""
import itertools
from collections import Counter

import numpy as np
import pytest

from tests import mesh_ref
from tests import world_mesh_cases as mc
from tests import world_mesh_ref as wmr

NORMALS = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], np.int64)


def world_cells(ref):
    """the world cell of every face"""
    f = ref["faces"]
    c = f["cell"].astype(np.int64)
    return ref["coords"].astype(np.int64)[f["brick"]] * 8 + np.stack([c & 7, (c >> 3) & 7, c >> 6], 1)


def check_expect(c, ref):
    info = ref["info"]
    for k, v in c["expect"].items():
        assert np.array_equal(np.asarray(info[k]), np.asarray(v)), (k, info[k], v)
    assert info["n_faces"] == len(ref["faces"]) == len(ref["quads"]) == info["faces_by_dir"].sum() == info["faces_by_kind"].sum()
    assert info["n_vertices"] == len(ref["corners"]) == len(ref["xyz"]) and info["n_bricks"] == len(ref["coords"])


def check_order(ref):
    """faces ascend in (brick, cell, dir), vertices in (owner brick in brick order, local word), each corner once and used"""
    f = ref["faces"]
    key = (f["brick"].astype(np.int64) << 12) | (f["cell"].astype(np.int64) << 3) | f["dir"]
    assert (np.diff(key) > 0).all()
    v = ref["corners"].astype(np.int64)
    own, loc = v >> 3, v & 7
    vk = [tuple(r) for r in np.concatenate([own[:, ::-1], loc[:, ::-1]], 1).tolist()]
    assert vk == sorted(vk) and len(set(vk)) == len(vk)
    assert len(ref["quads"]) == 0 or set(ref["quads"].reshape(-1).tolist()) == set(range(len(v)))


def check_normals(ref):
    """(q1 - q0) x (q3 - q0) is the outward unit normal of dir, q0 the smallest corner in (z, y, x), the quad the face's"""
    if not len(ref["faces"]):
        return
    q = ref["corners"].astype(np.int64)[ref["quads"].astype(np.int64)]          # [n, 4, 3]
    n = np.cross(q[:, 1] - q[:, 0], q[:, 3] - q[:, 0])
    d = ref["faces"]["dir"].astype(np.int64)
    assert np.array_equal(n, NORMALS[d])
    zyx = lambda p: (p[..., 2] << 42) + (p[..., 1] << 21) + p[..., 0]  # noqa: E731
    assert (zyx(q[:, 0] + (1 << 20))[:, None] <= zyx(q + (1 << 20))).all()
    # the four corners are the cell's face: on the plane cell + (dir odd), spanning the unit square
    cell = world_cells(ref)
    axis = d >> 1
    plane = cell[np.arange(len(d)), axis] + (d & 1)
    assert (q[np.arange(len(d)), :, axis] == plane[:, None]).all()
    assert np.array_equal(q.min(axis=1), cell + (NORMALS[d] > 0)) and np.array_equal(q.max(axis=1), cell + 1 - (NORMALS[d] < 0))


def check_closed(ref):
    """with no skip flag and no box every lattice edge carries 2 or 4 faces"""
    edges = Counter()
    for quad in ref["quads"].tolist():
        for a, b in zip(quad, quad[1:] + quad[:1]):
            edges[(min(a, b), max(a, b))] += 1
    assert set(edges.values()) <= {2, 4}, Counter(edges.values())


def check_divergence(ref):
    """the divergence theorem in integers: per axis (the field (x, 0, 0) has divergence 1) the sum over that axis' faces of
    sign x the face's coordinate along it is the number of solid cells"""
    d = ref["faces"]["dir"].astype(np.int64)
    cell = world_cells(ref)
    plane = cell[np.arange(len(d)), d >> 1] + (d & 1)
    for axis in range(3):
        on = (d >> 1) == axis
        assert int((np.where(d[on] & 1, 1, -1) * plane[on]).sum()) == int(ref["info"]["n_solid"]), axis


def both(c, **more):
    """the two restatements on a case: the same bytes"""
    kw = dict(c["kw"], **more)
    a = wmr.build_cells(c["hdr"], c["cells"], mc.MM, stamp=5, **kw)
    b = wmr.answer(wmr.BrickModel(c["hdr"], c["cells"], mc.MM, stamp=5, **kw))
    diff = wmr.difference(a, b)
    assert diff is None, diff
    return a


CRAFTED = mc.crafted()


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_archives(name):
    c = CRAFTED[name]
    ref = both(c)
    check_expect(c, ref), check_order(ref), check_normals(ref)
    kw = c["kw"]
    if not kw.get("skip_unknown_faces") and not kw.get("skip_absent_faces") and kw.get("box") is None:
        check_closed(ref), check_divergence(ref)


def test_the_crafted_cases_say_what_they_are_for():
    ref = both(CRAFTED["one cell at 7 7 7"])
    assert sorted(set(map(tuple, (ref["corners"] >> 3).tolist()))) == sorted(itertools.product((0, 1), repeat=3))   # seven the archive has not
    ref = both(CRAFTED["int16 edge"])
    assert ref["corners"].max() == 32768 * 8 and ref["corners"].min() == -32768 * 8 and (ref["faces"]["kind"] == 2).sum() == 6
    ref = both(CRAFTED["seam pair axis 0 label"])
    assert ref["faces"]["kind"][ref["faces"]["dir"] == 1].tolist() == [3]
    ref = both(CRAFTED["cube 2 x 2 x 2"])
    assert (ref["faces"]["kind"] == 2).all()                                     # no inner face
    parts = {k: both(CRAFTED["pillars " + k])["info"] for k in ("all", "static", "movable", "observed", "track 3")}
    assert parts["static"]["n_solid"] + parts["movable"]["n_solid"] == parts["all"]["n_solid"] == parts["observed"]["n_solid"]
    assert parts["track 3"]["n_solid"] == parts["movable"]["n_solid"] > 0 and parts["track 3"]["n_faces"] == parts["movable"]["n_faces"]


def test_the_random_archive_under_every_option():
    hdr, cells = mc.random_archive()
    c = dict(hdr=hdr, cells=cells, kw={})
    seen = set()
    for kw in mc.random_variants():
        ref = both(c, **kw)
        check_order(ref), check_normals(ref)
        if not kw["skip_unknown_faces"] and not kw["skip_absent_faces"] and kw["box"] is None:
            check_closed(ref), check_divergence(ref)
            assert (ref["info"]["faces_by_kind"][:3] > 0).all() and ref["info"]["n_bricks"] == 120
            assert (ref["info"]["faces_by_kind"][3] > 0) == bool(kw["observed_only"] or len(kw) > 4)
        seen.add(int(ref["info"]["options"]["flags"]))
    assert len(seen) == 48


def face_set(ref):
    return {(tuple(c), int(f["dir"])): (int(f["kind"]), int(f["track"]), int(f["label"]), int(f["occ"]))
            for c, f in zip(world_cells(ref).tolist(), ref["faces"])}


def test_disjoint_boxes_tile():
    hdr, cells = mc.random_archive()
    whole = wmr.answer(wmr.BrickModel(hdr, cells, mc.MM, observed_only=True))
    faces, corners = {}, set()
    boxes = mc.tiles_of((-1, -1, 0), (3, 3, 4), (1, 0, 2))
    assert len(boxes) == 8
    for box in boxes:
        part = wmr.answer(wmr.BrickModel(hdr, cells, mc.MM, observed_only=True, box=box))
        fs = face_set(part)
        assert len(fs) == len(part["faces"]) > 0 and not set(fs) & set(faces)
        faces.update(fs)
        corners |= set(map(tuple, part["corners"].tolist()))
    assert faces == face_set(whole) and corners == set(map(tuple, whole["corners"].tolist()))


@pytest.mark.parametrize("shape", [(8, 8, 16), (16, 16, 16)])
def test_a_fully_archived_box_is_the_block_mesh(shape):
    """a dense grid as a block (tests/mesh_ref.py) and as bricks: the same faces, corners and quads"""
    rng = np.random.default_rng(shape[2])
    u = rng.random(shape)
    g = np.full(shape, mc.FREE, np.uint32)
    g[u < 0.4], g[u < 0.25], g[u < 0.1], g[u < 0.05] = mc.UNKNOWN, mc.WALL, mc.GUESS, mc.MOVING
    lo = (-1, 3, -2)
    off = np.array(lo, np.int64) * 8
    hdr, cells = mc.from_grid(g, lo)
    for flags, kw in ((0, {}), (mesh_ref.STATIC_ONLY | mesh_ref.OBSERVED_ONLY, dict(static_only=True, observed_only=True)),
                      (mesh_ref.MOVABLE_ONLY | mesh_ref.SKIP_UNKNOWN_FACES, dict(movable_only=True, skip_unknown_faces=True)),
                      (mesh_ref.SKIP_BORDER_FACES, dict(skip_absent_faces=True))):
        block = mesh_ref.build(g, mc.MM, mesh_ref.options(flags=flags), fit=True)
        world = wmr.answer(wmr.BrickModel(hdr, cells, mc.MM, **kw))
        x_n, y_n = shape[2].bit_length() - 1, shape[1].bit_length() - 1
        w = block["faces"]["cell"].astype(np.int64)
        bcell = np.stack([w & (shape[2] - 1), (w >> x_n) & (shape[1] - 1), w >> (x_n + y_n)], 1) + off
        bf = {(tuple(c), int(f["dir"])): (int(f["kind"]), int(f["track"]), int(f["label"]), int(f["occ"])) for c, f in zip(bcell.tolist(), block["faces"])}
        assert bf == face_set(world) and len(bf) > 100
        bc = np.stack([block["corners"]["i"], block["corners"]["j"], block["corners"]["k"]], 1).astype(np.int64) + off
        assert set(map(tuple, bc.tolist())) == set(map(tuple, world["corners"].tolist()))
        bq = {(tuple(c), int(f["dir"])): bc[q].tolist() for c, f, q in zip(bcell.tolist(), block["faces"], block["quads"].astype(np.int64))}
        wq = {(tuple(c), int(f["dir"])): world["corners"][q].tolist()
              for c, f, q in zip(world_cells(world).tolist(), world["faces"], world["quads"].astype(np.int64))}
        assert bq == wq
