"""The crafted cases of the world rays tests: hand-written bricks (WORLD_BRICK headers in brick order and 512 words each)
with segments or views and their closed forms, shared by tests/test_world_rays_ref.py (the two restatements against each
other and against the closed forms, no GPU) and tests/test_world_rays_gpu.py (the library against them).  Every archive
feeds world_import on a fresh map of shape A, whose voxel_size is 1: a position IS its world-index coordinate.

A segment case: arch (hdr, cells), a, b, kw (unknown_blocks, ignore_movable), want - the fields of the one
WORLD_SEGMENT_HIT that the case states in closed form.  A view case: arch, views, dirs, reach, kw, want - fields of view 0's
VIEW_GAIN."""
import numpy as np

from semantic_dsp_map_amd import binding
from tests.world_reach_cases import CFG, FREE, MM, MOVING, UNKNOWN, WALL, bricks_of, from_grid  # noqa: F401

F = np.float32
SIZE = F(CFG["voxel_size"])
assert SIZE == 1.0
MID = (3.5, 3.5)                       # y and z of the axis-aligned rays: cell centres
IDENTITY = (1.0, 0.0, 0.0, 0.0)


def t32(plane, a, b):
    """the t of a crossing as the walk computes it: (plane - u_a) * (1 / (u_b - u_a)) in double, then float32"""
    return F((float(plane) - float(F(a))) * (1.0 / (float(F(b)) - float(F(a)))))


def row(n_bricks, walls=(), skip=(), lo=0, moving=()):
    """bricks lo .. lo + n_bricks - 1 in a row along x, free; `walls` / `moving`: planes x = const of WALL / MOVING words"""
    g = np.full((8, 8, 8 * n_bricks), FREE, np.uint32)
    for x in walls:
        g[:, :, x - 8 * lo] = WALL
    for x in moving:
        g[:, :, x - 8 * lo] = MOVING
    return from_grid(g, (lo, 0, 0), skip=[(s, 0, 0) for s in skip])


def seg(arch, a, b, want, **kw):
    return dict(arch=arch, a=np.array(a, F), b=np.array(b, F), kw=kw, want=want)


def along_x(x0, x1):
    return (x0,) + MID, (x1,) + MID


def segment_cases():
    out = {}
    # an axis-aligned ray through cell centres across a brick seam into a wall: cells 0 .. 12
    out["seam into a wall"] = seg(row(2, walls=[12]), *along_x(0.5, 15.5), dict(t=t32(12, 0.5, 15.5), cells=13, cell=(12, 3, 3), occ=1, track=65535,
                                                                                 label=8, unknown=0, stamp=1))
    # the same across an absent brick between two archived ones: its eight cells are unknown; with UNKNOWN_BLOCKS the ray
    # is blocked at the absent brick's first cell
    gap = row(3, walls=[20], skip=[1])
    out["across an absent brick"] = seg(gap, *along_x(0.5, 23.5), dict(t=t32(20, 0.5, 23.5), cells=21, cell=(20, 3, 3), occ=1, unknown=8, stamp=1))
    out["blocked at an absent brick"] = seg(gap, *along_x(0.5, 23.5), dict(t=t32(8, 0.5, 23.5), cells=9, cell=(8, 3, 3), occ=-1, track=0, label=0,
                                                                            unknown=1, stamp=0), unknown_blocks=True)
    # a diagonal through the corner where eight bricks meet: all three planes at t = 0.5, x steps before y before z, so the
    # cells are (-1, -1, -1), (0, -1, -1), (0, 0, -1), (0, 0, 0)
    g = np.full((16, 16, 16), FREE, np.uint32)
    eight = from_grid(g, (-1, -1, -1))
    out["diagonal through a corner"] = seg(eight, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), dict(t=-1.0, cells=4, cell=(0, 0, 0), occ=-1, unknown=0))
    g = g.copy()
    g[7, 7, 8] = WALL                                   # (0, -1, -1): the second cell under x before y
    out["diagonal, wall after the x step"] = seg(from_grid(g, (-1, -1, -1)), (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5),
                                                 dict(t=F(0.5), cells=2, cell=(0, -1, -1), occ=1))
    g = np.full((16, 16, 16), FREE, np.uint32)
    g[7, 8, 7] = WALL                                   # (-1, 0, -1): visited only if y stepped first
    out["diagonal, wall beside the path"] = seg(from_grid(g, (-1, -1, -1)), (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), dict(t=-1.0, cells=4))
    # a ray ending exactly on a plane: going up the plane at t = 1 is crossed into the cell of b, cells 1 .. 5; going down
    # the plane under a is crossed at t = 0 and the plane at t = 1 as well: cells 5, 4, 3, 2, 1, 0
    one = row(1)
    out["ends on a plane, going up"] = seg(one, *along_x(1.0, 5.0), dict(t=-1.0, cells=5, unknown=0))
    out["ends on a plane, going down"] = seg(one, *along_x(5.0, 1.0), dict(t=-1.0, cells=6, unknown=0))
    # a zero-length segment is the cell of a
    out["zero length, free"] = seg(one, (3.5, 3.5, 3.5), (3.5, 3.5, 3.5), dict(t=-1.0, cells=1, unknown=0))
    out["zero length, in a wall"] = seg(row(1, walls=[3]), (3.5, 3.5, 3.5), (3.5, 3.5, 3.5), dict(t=F(0), cells=1, cell=(3, 3, 3), occ=1, stamp=1))
    # a negative-coordinate seam: cells -1 and 0 are bricks -1 and 0
    neg = row(2, walls=[-1], lo=-1)
    out["negative seam"] = seg(neg, *along_x(0.5, -2.5), dict(t=t32(0, 0.5, -2.5), cells=2, cell=(-1, 3, 3), occ=1))
    out["starts below zero"] = seg(neg, *along_x(-0.5, -2.5), dict(t=F(0), cells=1, cell=(-1, 3, 3), occ=1))   # floor(-0.5) = -1, not 0
    # a movable wall before a static one
    mov = row(2, walls=[7], moving=[5])
    out["movable wall"] = seg(mov, *along_x(0.5, 15.5), dict(t=t32(5, 0.5, 15.5), cells=6, cell=(5, 3, 3), occ=1, track=3, label=7))
    out["movable wall ignored"] = seg(mov, *along_x(0.5, 15.5), dict(t=t32(7, 0.5, 15.5), cells=8, cell=(7, 3, 3), occ=1, track=65535),
                                      ignore_movable=True)
    # invalid inputs
    invalid, blocked = dict(t=-1.0, cells=0, cell=(0, 0, 0), occ=-1, track=0, unknown=0, stamp=0), dict(t=F(0), cells=0, cell=(0, 0, 0), occ=-1, unknown=0)
    out["NaN end point"] = seg(one, (0.5, np.nan, 0.5), (3.5, 0.5, 0.5), invalid)
    out["NaN end point blocks"] = seg(one, (0.5, 0.5, 0.5), (3.5, 0.5, np.inf), blocked, unknown_blocks=True)
    out["beyond the brick range"] = seg(one, (0.5, 0.5, 0.5), (262144.5, 0.5, 0.5), invalid)
    out["beyond the brick range blocks"] = seg(one, (0.5, -262144.5, 0.5), (0.5, 0.5, 0.5), blocked, unknown_blocks=True)
    out["8192 cells are walked"] = seg(one, (0.5, 0.5, 0.5), (8191.5, 0.5, 0.5), dict(t=-1.0, cells=8192, unknown=8184))
    out["8193 cells are too long"] = seg(one, (0.5, 0.5, 0.5), (8192.5, 0.5, 0.5), dict(t=-1.0, cells=-1, cell=(0, 0, 0), occ=-1, unknown=0, stamp=0))
    out["too long under any flag"] = seg(one, (0.5, 0.5, 0.5), (4000.5, 4000.5, 200.5), dict(t=-1.0, cells=-1, unknown=0), unknown_blocks=True)
    # at the int16 edge: the walk's last step, across the plane at t = 1, leaves the brick range; that cell is absent
    out["over the edge of the brick range"] = seg(one, (-262142.0, 0.5, 0.5), (-262144.0, 0.5, 0.5), dict(t=-1.0, cells=4, unknown=4))
    # a hit in the first cell
    out["hit in the first cell"] = seg(row(1, walls=[0]), *along_x(0.5, 6.5), dict(t=F(0), cells=1, cell=(0, 3, 3), occ=1))
    # a batch of the walk is eight cells: a wall at the 8th, the 9th and the 17th cell
    for nth in (8, 9, 17):
        out["wall at cell %d" % nth] = seg(row(3, walls=[nth - 1]), *along_x(0.5, 23.5), dict(t=t32(nth - 1, 0.5, 23.5), cells=nth, cell=(nth - 1, 3, 3)))
    return out


# ---- views -----------------------------------------------------------------------------------------------------------
PINHOLE = binding.pinhole_rays(dict(width=16, height=12, cx=7.5, cy=5.5, fx=10.0, fy=10.0)).reshape(-1, 3)   # 192 rays
ONE_RAY = np.array([[0.0, 0.0, 1.0]], F)
WAVE_AND_ONE = np.repeat(ONE_RAY, 65, axis=0)                      # 65 rays that share every cell


def view(pos, rng, q=IDENTITY):
    v = np.zeros(1, binding.VIEW)
    v["pos"], v["q"], v["range"] = pos, q, rng
    return v


def room():
    """3 x 3 x 3 bricks round (0, 0, 0), free, a wall in the plane z = 12, unknown cells in the plane z = 9; beyond: absent"""
    g = np.full((24, 24, 24), FREE, np.uint32)
    g[8 + 12] = WALL
    g[8 + 9, ::2, ::2] = UNKNOWN
    return from_grid(g, (-1, -1, -1))


def views_case(arch, views, dirs, reach, want=None, **kw):
    return dict(arch=arch, views=np.asarray(views, binding.VIEW).reshape(-1), dirs=np.asarray(dirs, F).reshape(-1, 3), reach=reach, kw=kw, want=want or {})


def view_cases():
    out = {}
    r, eye = room(), (3.5, 3.5, 3.5)
    # one ray up the z axis from cell (3, 3, 3): z = 3 .. 11 free (z = 9 at odd x, y is free), the wall at z = 12
    out["one ray, reach 20"] = views_case(r, view(eye, 15.0), ONE_RAY, 20, dict(n_free=9, n_unknown=0, n_occupied=1, rays_hit=1, rays_in_map=1, ray_cells=10,
                                                                                ray_unknown=0))
    out["one ray, reach 4"] = views_case(r, view(eye, 15.0), ONE_RAY, 4, dict(n_free=5, n_occupied=0, rays_hit=0, rays_in_map=1, ray_cells=5))   # z = 3 .. 7
    out["one ray, reach 1"] = views_case(r, view(eye, 15.0), ONE_RAY, 1, dict(n_free=2, n_occupied=0, rays_hit=0, ray_cells=2))
    # 65 rays that share all their cells: 65 x 6 cells visited, 6 distinct
    out["shared cells"] = views_case(r, view(eye, 5.0), WAVE_AND_ONE, 20, dict(n_free=6, n_unknown=0, n_occupied=0, rays_in_map=65, ray_cells=390, rays_hit=0))
    # ... and into the absent bricks above the room: z = 3 .. 15 archived (the wall ignored: the ray starts behind it)
    out["into absent bricks"] = views_case(r, view((3.5, 3.5, 13.5), 10.0), WAVE_AND_ONE, 20, dict(n_free=3, n_unknown=8, n_occupied=0, ray_cells=65 * 11,
                                                                                                    ray_unknown=65 * 8, rays_in_map=65))
    for reach in (1, 4, 20):
        out["pinhole, reach %d" % reach] = views_case(r, view(eye, 15.0), PINHOLE, reach)
    # a window that cuts rays short: no ray of the pinhole table reaches the wall within four cells
    out["pinhole cut short"] = views_case(r, view(eye, 30.0), PINHOLE, 4, dict(rays_hit=0, n_occupied=0, rays_in_map=192))
    # several views, one of them turned, one with range 0, one non-finite
    vs = np.concatenate([view(eye, 15.0), view((-3.5, 2.5, 1.5), 12.0, q=(0.70710678, 0.0, 0.70710678, 0.0)), view(eye, 0.0), view((np.nan, 0, 0), 5.0),
                         view(eye, 8.0, q=(np.inf, 0, 0, 0))])
    out["several views"] = views_case(r, vs, PINHOLE, 20)
    # a window that reaches beyond the int16 brick range makes the view invalid; one cell further in it is valid
    out["window at the edge"] = views_case(r, view((262143.5 - 19, 0.5, 0.5), 5.0), ONE_RAY, 20, dict(n_free=0, n_unknown=0, rays_in_map=0, ray_cells=0))
    out["window inside the edge"] = views_case(r, view((262143.5 - 20, 0.5, 0.5), 5.0), ONE_RAY, 20, dict(n_unknown=6, rays_in_map=1, ray_cells=6))
    # a non-finite ray among finite ones invalidates that ray only
    d = PINHOLE[:65].copy()
    d[7, 1] = np.nan
    out["one bad ray"] = views_case(r, view(eye, 15.0), d, 20, dict(rays_in_map=64))
    # movable cells: the wall of the room is static, a movable plate stands before it
    g = np.full((24, 24, 24), FREE, np.uint32)
    g[8 + 12], g[8 + 6] = WALL, MOVING
    plate = from_grid(g, (-1, -1, -1))
    out["movable plate"] = views_case(plate, view(eye, 15.0), ONE_RAY, 20, dict(n_free=3, n_occupied=1, ray_cells=4))
    out["movable plate ignored"] = views_case(plate, view(eye, 15.0), ONE_RAY, 20, dict(n_free=9, n_occupied=1, ray_cells=10), ignore_movable=True)
    return out


# ---- random: 4 x 4 x 3 bricks with holes, about 10 % obstacles, some of them movable, some unknown cells -----------------
RANDOM_SKIP = [(0, 1, 0), (2, 2, 1), (-1, 0, 2), (1, -1, 1)]


def random_archive(seed=23):
    rng = np.random.default_rng(seed)
    u = rng.random((24, 32, 32))
    g = np.full(u.shape, FREE, np.uint32)
    g[u < 0.2] = UNKNOWN
    g[u < 0.1] = WALL
    g[u < 0.03] = MOVING
    return from_grid(g, (-1, -1, 0), skip=RANDOM_SKIP)


def random_segments(n=512, seed=29):
    """end points in and round the archive (cells -8 .. 24 in x and y, 0 .. 24 in z), a few far away"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-12.0, -12.0, -4.0]), np.array([28.0, 28.0, 28.0])
    a = (lo + rng.random((n, 3)) * (hi - lo)).astype(F)
    b = (lo + rng.random((n, 3)) * (hi - lo)).astype(F)
    b[::16] = a[::16] + (rng.random((len(b[::16]), 3)) * 400 - 200).astype(F)     # long ones, through absent space
    b[5::64, 1] = a[5::64, 1]                                                       # parallel to an axis plane
    b[9::64] = a[9::64]                                                             # zero length
    return a, b


def random_views(n=12, seed=37):
    rng = np.random.default_rng(seed)
    v = np.zeros(n, binding.VIEW)
    v["pos"] = (np.array([-4.0, -4.0, 2.0]) + rng.random((n, 3)) * np.array([24.0, 24.0, 20.0])).astype(F)
    q = rng.standard_normal((n, 4))
    v["q"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    v["range"] = (4.0 + rng.random(n) * 20.0).astype(F)
    return v
