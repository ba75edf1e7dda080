"""tests/mesh_ref.py held to plain triple loops and to invariants that do not share its code: the restatement the GPU test
compares against is itself checked on the CPU.  Also binding.mesh_triangles and binding.write_ply, which are host code."""
import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import mesh_ref as mr

MAX_MOVABLE = 10
SHAPE = (16, 4, 8)     # [z, y, x]: 8 x 4 x 16 cells


def word(occ, label, track):
    return (np.asarray(track, np.uint32) & 0xFFFF) | (np.asarray(label, np.uint32) << 16) | ((np.asarray(occ, np.int64) & 0xFF).astype(np.uint32) << 24)


def random_snap(seed, shape=SHAPE, p_solid=0.3):
    rng = np.random.default_rng(seed)
    occ = rng.choice(np.array([-1, 0, 1, 2]), size=shape, p=[0.2, 0.8 - p_solid, p_solid * 0.7, p_solid * 0.3])
    label = rng.choice(np.array([3, 7, 200]), size=shape)
    track = rng.choice(np.array([0, 4, 10, 11, 500]), size=shape)
    return word(occ, label, track)


def loops(snap, max_movable, opt):
    """the contract, cell by cell: -> (faces as tuples, quads as corner triples, the vertex list)"""
    NZ, NY, NX = snap.shape
    x_n, y_n = NX.bit_length() - 1, NY.bit_length() - 1
    f = opt["flags"]

    def parts(i, j, k):
        w = int(snap[k, j, i])
        occ = (w >> 24) & 0xFF
        return (occ - 256 if occ >= 128 else occ), (w >> 16) & 0xFF, w & 0xFFFF

    def solid(i, j, k):
        occ, label, track = parts(i, j, k)
        if not (occ == 1 if f & mr.OBSERVED_ONLY else occ >= 1):
            return False
        if opt["labels"] is not None and label not in opt["labels"]:
            return False
        if opt["track"] != -1 and track != opt["track"]:
            return False
        movable = 1 <= track <= max_movable
        return not ((f & mr.STATIC_ONLY and movable) or (f & mr.MOVABLE_ONLY and not movable))

    faces, quad_corners = [], []
    for k in range(NZ):
        for j in range(NY):
            for i in range(NX):
                if not solid(i, j, k):
                    continue
                for d, (axis, step) in enumerate(mr.DIRS):
                    n = [i, j, k]
                    n[axis] += step
                    if not (0 <= n[0] < NX and 0 <= n[1] < NY and 0 <= n[2] < NZ):
                        kind = 2
                    elif solid(*n):
                        continue
                    else:
                        o = parts(*n)[0]
                        kind = 1 if o == -1 else (0 if o == 0 else 3)
                    if (kind == 1 and f & mr.SKIP_UNKNOWN_FACES) or (kind == 2 and f & mr.SKIP_BORDER_FACES):
                        continue
                    occ, label, track = parts(i, j, k)
                    faces.append((i | (j << x_n) | (k << (x_n + y_n)), track, label, occ, d, kind, 0))
                    quad_corners.append([(i + a, j + b, k + c) for a, b, c in mr.QUAD[d].tolist()])
    used = sorted({c for q in quad_corners for c in q}, key=lambda c: c[0] + (NX + 1) * (c[1] + (NY + 1) * c[2]))
    index = {c: n for n, c in enumerate(used)}
    return faces, [[index[c] for c in q] for q in quad_corners], used


OPTION_SETS = [mr.options(), mr.options(flags=mr.STATIC_ONLY), mr.options(flags=mr.MOVABLE_ONLY | mr.OBSERVED_ONLY),
               mr.options(flags=mr.SKIP_UNKNOWN_FACES), mr.options(flags=mr.SKIP_BORDER_FACES | mr.SKIP_UNKNOWN_FACES),
               mr.options(labels=[3, 200]), mr.options(track=4), mr.options(track=500, labels=[7]), mr.options(labels=[]),
               mr.options(track=9)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_triple_loops(seed):
    snap = random_snap(seed)
    kinds = set()
    for opt in OPTION_SETS:
        got = mr.build(snap, MAX_MOVABLE, dict(opt, max_faces=6 * snap.size), 0.25, (1.0, -2.0, 3.5))   # (room for every face)
        faces, quads, used = loops(snap, MAX_MOVABLE, opt)
        assert [tuple(int(v) for v in r) for r in got["faces"]] == faces, opt
        assert got["quads"].tolist() == quads, opt
        assert [(int(c["i"]), int(c["j"]), int(c["k"])) for c in got["corners"]] == used and (got["corners"]["pad"] == 0).all()
        info = got["info"]
        assert info["n_faces"] == len(faces) and info["n_vertices"] == len(used)
        assert info["faces_by_dir"].tolist() == [sum(1 for r in faces if r[4] == d) for d in range(6)]
        assert info["faces_by_kind"].tolist() == [sum(1 for r in faces if r[5] == k) for k in range(4)]
        want_xyz = [[np.float32(o) + np.float32(c) * np.float32(0.25) for o, c in zip((1.0, -2.0, 3.5), u)] for u in used]
        assert got["xyz"].tolist() == [[float(v) for v in p] for p in want_xyz]
        kinds |= set(r[5] for r in faces)
    assert kinds == {0, 1, 2, 3}
    assert not mr.build(snap, MAX_MOVABLE, mr.options(labels=[]))["info"]["n_faces"]
    assert not mr.build(snap, MAX_MOVABLE, mr.options(track=9))["info"]["n_solid"]


def corner_words(mesh, shape):
    NZ, NY, NX = shape
    c = mesh["corners"]
    return c["i"].astype(np.int64) + (NX + 1) * (c["j"].astype(np.int64) + (NY + 1) * c["k"].astype(np.int64))


def cells_of(faces, shape):
    NZ, NY, NX = shape
    x_n, y_n = NX.bit_length() - 1, NY.bit_length() - 1
    c = faces["cell"].astype(np.int64)
    return np.stack([c & (NX - 1), (c >> x_n) & (NY - 1), c >> (x_n + y_n)], axis=1)


def check_invariants(mesh, shape, closed):
    faces, quads, corners = mesh["faces"], mesh["quads"].astype(np.int64), mesh["corners"]
    p = np.stack([corners["i"], corners["j"], corners["k"]], axis=1).astype(np.int64)
    q = p[quads]                                              # [n, 4, 3]
    assert np.array_equal(np.cross(q[:, 1] - q[:, 0], q[:, 3] - q[:, 0]), mr.NORMALS[faces["dir"]])
    cw = corner_words(mesh, shape)
    assert (np.diff(cw) > 0).all()                            # each corner once, ascending
    assert (cw[quads[:, 0]][:, None] <= cw[quads]).all()      # q0 is the smallest corner word
    assert np.array_equal(np.unique(quads), np.arange(len(corners)))   # every vertex is used
    key = faces["cell"].astype(np.int64) * 6 + faces["dir"]
    assert (np.diff(key) > 0).all()
    # the divergence theorem in integers, per axis
    cell = cells_of(faces, shape)
    for a in range(3):
        plus, minus = faces["dir"] == 2 * a + 1, faces["dir"] == 2 * a
        if closed:
            assert int((cell[plus, a] + 1).sum() - cell[minus, a].sum()) == int(mesh["info"]["n_solid"])
    if closed:                                                # every lattice edge carries 2 or 4 faces
        edges = np.concatenate([np.stack([quads[:, e], quads[:, (e + 1) % 4]], axis=1) for e in range(4)])
        edges.sort(axis=1)
        _, count = np.unique(edges, axis=0, return_counts=True)
        assert set(count.tolist()) <= {2, 4}, set(count.tolist())
    tri = binding.mesh_triangles(mesh["quads"])
    assert tri.shape == (2 * len(faces), 3)
    assert np.array_equal(tri[0::2], mesh["quads"][:, [0, 1, 2]]) and np.array_equal(tri[1::2], mesh["quads"][:, [0, 2, 3]])


@pytest.mark.parametrize("seed", [4, 5])
def test_invariants(seed):
    snap = random_snap(seed, p_solid=0.45)
    for opt in OPTION_SETS:
        mesh = mr.build(snap, MAX_MOVABLE, opt)
        check_invariants(mesh, SHAPE, closed=not (opt["flags"] & (mr.SKIP_UNKNOWN_FACES | mr.SKIP_BORDER_FACES)))


def test_small_bodies():
    free = word(np.zeros(SHAPE, np.int64), 0, 0)
    one = free.copy()
    one[5, 2, 3] = word(1, 7, 0)
    m = mr.build(one, MAX_MOVABLE, mr.options())
    assert m["info"]["n_faces"] == 6 and m["info"]["n_vertices"] == 8 and m["info"]["faces_by_kind"].tolist() == [6, 0, 0, 0]
    assert m["faces"]["dir"].tolist() == [0, 1, 2, 3, 4, 5] and (m["faces"]["cell"] == 3 | (2 << 3) | (5 << 5)).all()
    for axis in range(3):
        two = one.copy()
        n = [3, 2, 5]
        n[axis] += 1
        two[n[2], n[1], n[0]] = word(2, 7, 0)
        m = mr.build(two, MAX_MOVABLE, mr.options())
        assert m["info"]["n_faces"] == 10 and m["info"]["n_vertices"] == 12 and m["info"]["n_solid"] == 2
        check_invariants(m, SHAPE, closed=True)
        m = mr.build(two, MAX_MOVABLE, mr.options(flags=mr.OBSERVED_ONLY))   # the guessed cell is a kind-3 neighbour now
        assert m["info"]["n_faces"] == 6 and m["info"]["faces_by_kind"].tolist() == [5, 0, 0, 1]
    NZ, NY, NX = SHAPE
    full = word(np.ones(SHAPE, np.int64), 7, 0)
    m = mr.build(full, MAX_MOVABLE, mr.options(max_faces=6 * NX * NY * NZ))
    assert m["info"]["n_faces"] == 2 * (NX * NY + NY * NZ + NX * NZ) and (m["faces"]["kind"] == 2).all() and not m["over"]
    check_invariants(m, SHAPE, closed=True)
    assert mr.build(full, MAX_MOVABLE, mr.options(flags=mr.SKIP_BORDER_FACES))["info"]["n_faces"] == 0
    corner = free.copy()
    corner[0, 0, 0] = corner[NZ - 1, NY - 1, NX - 1] = word(1, 7, 0)
    m = mr.build(corner, MAX_MOVABLE, mr.options())
    assert m["info"]["faces_by_kind"].tolist() == [6, 0, 6, 0]


def test_capacities_and_the_info_of_a_build_over_them():
    z, y, x = np.indices(SHAPE)
    board = word(((x + y + z) & 1).astype(np.int64), 7, 0)
    V = board.size
    n_corners = 9 * 5 * 17
    n_used = n_corners - 4    # every corner but the four corners of the map whose only cell is free
    m = mr.build(board, MAX_MOVABLE, mr.options())
    assert m["over"] and m["info"]["n_faces"] == 3 * V and m["info"]["n_vertices"] == n_used
    assert m["info"]["faces_by_dir"].sum() == 0 and m["info"]["options"]["max_faces"] == V // 8 and m["info"]["options"]["max_vertices"] == V // 8 + V // 16
    m = mr.build(board, MAX_MOVABLE, mr.options(max_faces=3 * V, max_vertices=10 ** 9))
    assert not m["over"] and m["info"]["options"]["max_vertices"] == n_corners and m["info"]["faces_by_dir"].tolist() == [V // 2] * 6
    assert not mr.build(board, MAX_MOVABLE, mr.options(max_faces=3 * V, max_vertices=n_used))["over"]
    assert mr.build(board, MAX_MOVABLE, mr.options(max_faces=3 * V, max_vertices=n_used - 1))["over"]
    assert mr.build(board, MAX_MOVABLE, mr.options(max_faces=3 * V - 1, max_vertices=n_used))["over"]
    assert mr.capacities(mr.options(max_faces=10 ** 12), V, 1)[0] == 6 * V and mr.capacities(mr.options(), 4, 100) == (1, 1)


def read_ply(path):
    """a small parser of what write_ply writes -> (xyz float32 [m, 3], triangles [t, 3], rgb [t, 3] or None)"""
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    end = lines.index("end_header")
    head = lines[2:end]
    n_v = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    n_f = int([h for h in head if h.startswith("element face")][0].split()[-1])
    coloured = "property uchar red" in head
    body = lines[end + 1:]
    assert body[-1] == "" and len(body) == n_v + n_f + 1
    xyz = np.array([[np.float32(v) for v in l.split()] for l in body[:n_v]], np.float32).reshape(-1, 3)
    rows = [[int(v) for v in l.split()] for l in body[n_v:n_v + n_f]]
    assert all(r[0] == 3 and len(r) == (7 if coloured else 4) for r in rows)
    tri = np.array([r[1:4] for r in rows], np.int64).reshape(-1, 3)
    return xyz, tri, (np.array([r[4:] for r in rows], np.int64) if coloured else None)


def test_write_ply_round_trips(tmp_path):
    snap = random_snap(6)
    m = mr.build(snap, MAX_MOVABLE, mr.options(), 0.1, (123.456, -0.3, 1e-3))
    rgb = np.stack([m["faces"]["label"], m["faces"]["dir"] * 40, m["faces"]["kind"] * 80], axis=1)
    for colours in (None, rgb):
        path = str(tmp_path / "mesh.ply")
        binding.write_ply(path, m["xyz"], m["quads"], colours)
        xyz, tri, got_rgb = read_ply(path)
        assert xyz.tobytes() == m["xyz"].tobytes() and np.array_equal(tri, binding.mesh_triangles(m["quads"]))
        assert (got_rgb is None) if colours is None else np.array_equal(got_rgb, np.repeat(rgb, 2, axis=0))
    binding.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 4), np.uint32))
    xyz, tri, _ = read_ply(str(tmp_path / "empty.ply"))
    assert len(xyz) == 0 and len(tri) == 0
    with pytest.raises(ValueError):
        binding.write_ply(path, m["xyz"], m["quads"], rgb[:-1])
