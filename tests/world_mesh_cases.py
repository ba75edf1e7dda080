"""The crafted archives of the world mesh tests: the smallest ones that show one way to go wrong each, with closed-form
expectations, shared by tests/test_world_mesh_ref.py (the two restatements against each other and against checks of their
own, no GPU) and tests/test_world_mesh_gpu.py (the library against the model).  A case is a dict: hdr, cells (WORLD_BRICK
headers in brick order, 512 words each), kw (the build's keywords) and expect (info fields -> value)."""
import itertools

import numpy as np

from tests.world_reach_cases import CFG, FREE, MM, MOVING, UNKNOWN, WALL, ball, bricks_of, from_grid, int16_edge, pillars  # noqa: F401

WALL9 = 1 << 24 | 9 << 16 | 65535     # occupied, static, another label
GUESS = 2 << 24 | 8 << 16 | 65535     # guessed occupied (occ == 2)


def case(hdr_cells, expect=None, **kw):
    return dict(hdr=hdr_cells[0], cells=hdr_cells[1], kw=kw, expect=expect or {})


def free_brick():
    return np.full((8, 8, 8), FREE, np.uint32)


def one_cell(c):
    g = free_brick()
    g[c[2], c[1], c[0]] = WALL
    nvb = 2 ** sum(1 for v in c if v == 7)
    return case(bricks_of({(0, 0, 0): g}), dict(n_faces=6, n_vertices=8, n_vertex_bricks=nvb, n_solid=1, n_bricks=1, faces_by_dir=[1] * 6))


def x_wrap():
    """(cx 7, cy 2) and (cx 0, cy 3) are neighbours in the slice's word and not in space"""
    g = free_brick()
    g[3, 2, 7] = g[3, 3, 0] = WALL
    return case(bricks_of({(0, 0, 0): g}), dict(n_faces=12, n_vertices=16, n_solid=2))


def seam_pair(axis, variant):
    """two solid cells face each other across the seam between brick 0 and the next brick along `axis`"""
    a, b = free_brick(), free_brick()
    ia, ib = [3, 3, 3], [3, 3, 3]            # (cx, cy, cz)
    ia[axis], ib[axis] = 7, 0
    a[ia[2], ia[1], ia[0]] = WALL
    b[ib[2], ib[1], ib[0]] = WALL9 if variant == "label" else WALL
    nxt = [0, 0, 0]
    nxt[axis] = 1
    arch = bricks_of({(0, 0, 0): a, tuple(nxt): b})
    if variant == "box":
        return case(arch, dict(n_faces=5, n_vertices=8, n_solid=1, n_bricks=1, faces_by_kind=[5, 0, 0, 0]), box=((0, 0, 0), (0, 0, 0)))
    if variant == "label":
        return case(arch, dict(n_faces=6, n_vertices=8, n_solid=1, n_bricks=2, faces_by_kind=[5, 0, 0, 1]), labels=[8])
    return case(arch, dict(n_faces=10, n_vertices=12, n_solid=2, n_bricks=2, faces_by_kind=[10, 0, 0, 0]))


def kinds(skip_unknown, skip_absent):
    """one solid cell at the +x face of its brick: free behind -x and -z, unknown behind -y and +z, no brick behind +x, an
    occupied cell of another label behind +y"""
    g = free_brick()
    g[3, 3, 7] = WALL
    g[3, 2, 7] = g[4, 3, 7] = UNKNOWN
    g[3, 4, 7] = MOVING
    by_kind = [2, 0 if skip_unknown else 2, 0 if skip_absent else 1, 1]
    by_dir = [1, 0 if skip_absent else 1, 0 if skip_unknown else 1, 1, 1, 0 if skip_unknown else 1]
    return case(bricks_of({(0, 0, 0): g}), dict(n_faces=sum(by_kind), faces_by_kind=by_kind, faces_by_dir=by_dir, n_solid=1), labels=[8],
                skip_unknown_faces=skip_unknown, skip_absent_faces=skip_absent)


def edge_cells():
    """the int16 edge: every brick at +32767 / -32768 has a solid cell at local 7 / 0 on that axis - its corners belong to
    owner 32768 / its face looks at a brick beyond the range"""
    c = int16_edge()
    cells = c["cells"].copy().reshape(-1, 8, 8, 8)
    n = 0
    for i, h in enumerate(c["hdr"]):
        b = [int(h["bx"]), int(h["by"]), int(h["bz"])]
        if tuple(b) in c["lonely"]:
            continue
        a = [k for k in range(3) if b[k] in (32767, -32768)][0]
        at = [3, 3, 3]
        at[a] = 7 if b[a] == 32767 else 0
        cells[i, at[2], at[1], at[0]] = WALL
        n += 1
    assert n == 6
    return case((c["hdr"], cells.reshape(-1, 512)), dict(n_faces=36, n_vertices=48, n_solid=6, faces_by_kind=[30, 0, 6, 0], n_bricks=12))


def cube(nb):
    g = np.full((8 * nb,) * 3, WALL, np.uint32)
    side = 8 * nb
    return case(from_grid(g, (-1, 2, -3)), dict(n_faces=6 * side * side, n_vertices=(side + 1) ** 3 - (side - 1) ** 3, n_solid=side ** 3,
                                                n_vertex_bricks=(nb + 1) ** 3 - (nb - 1) ** 3 if nb > 1 else 8, faces_by_kind=[0, 0, 6 * side * side, 0]))


def checkerboard():
    z, y, x = np.indices((8, 8, 8))
    g = np.where((x + y + z) % 2 == 0, WALL, FREE).astype(np.uint32)
    return case(bricks_of({(4, -4, 0): g}), dict(n_faces=1536, n_vertices=725, n_vertex_bricks=7, n_solid=256))   # (every corner but the four brick vertices at a free cell, (8, 8, 8) among them)


def ball_case(skip):
    c = ball(1, skip)
    return case((c["hdr"], c["cells"]), dict(n_faces=6, n_vertices=8, n_vertex_bricks=1, n_solid=1, n_bricks=7 if skip else 8, faces_by_kind=[6, 0, 0, 0]))


def pillars_case(**kw):
    c = pillars(1, False)
    return case((c["hdr"], c["cells"]), None, **kw)


def crafted():
    out = {"one cell at 0 0 0": one_cell((0, 0, 0)), "one cell at 7 7 7": one_cell((7, 7, 7)), "one cell at 7 0 3": one_cell((7, 0, 3)),
           "ball": ball_case(False), "ball, a brick skipped": ball_case(True), "x wrap": x_wrap(), "int16 edge": edge_cells(), "cube": cube(1),
           "cube 2 x 2 x 2": cube(2), "checkerboard": checkerboard()}
    for axis, variant in itertools.product(range(3), ("plain", "box", "label")):
        out["seam pair axis %d %s" % (axis, variant)] = seam_pair(axis, variant)
    for su, sa in itertools.product((False, True), (False, True)):
        out["kinds skip_unknown=%s skip_absent=%s" % (su, sa)] = kinds(su, sa)
    for name, kw in (("all", {}), ("static", dict(static_only=True)), ("movable", dict(movable_only=True)), ("observed", dict(observed_only=True)),
                     ("track 3", dict(track=3))):
        out["pillars " + name] = pillars_case(**kw)
    return out


# ---- the random archive: 5 x 5 x 5 bricks, five missing
RANDOM_SKIP = [(0, 0, 0), (1, 1, 1), (-1, 2, 0), (3, -1, 2), (2, 3, 4)]
RANDOM_BOX = ((0, -1, 1), (2, 1, 3))


def random_archive(seed=21):
    rng = np.random.default_rng(seed)
    u = rng.random((40, 40, 40))
    g = np.full(u.shape, FREE, np.uint32)
    g[u < 0.40] = UNKNOWN
    g[u < 0.20] = WALL
    g[u < 0.10] = WALL9
    g[u < 0.06] = GUESS
    g[u < 0.03] = MOVING
    return from_grid(g, (-1, -1, 0), skip=RANDOM_SKIP)


def random_variants():
    """every legal flag combination, without and with a box; some with a label mask"""
    out = []
    for mode, obs, su, sa, box in itertools.product((None, "static_only", "movable_only"), (False, True), (False, True), (False, True),
                                                    (None, RANDOM_BOX)):
        kw = dict(observed_only=obs, skip_unknown_faces=su, skip_absent_faces=sa, box=box)
        if mode:
            kw[mode] = True
        if su != sa:
            kw["labels"] = [7, 8]
        out.append(kw)
    return out


def tiles_of(lo, hi, cut):
    """disjoint brick boxes that cover lo .. hi: split at `cut` on every axis"""
    spans = [((lo[a], cut[a]), (cut[a] + 1, hi[a])) for a in range(3)]
    return [tuple(zip(*pick)) for pick in itertools.product(*spans)]
