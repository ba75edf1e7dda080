"""Scenarios that hold the oracle and the HIP library to the reference's own ring buffer (mc_ring/*.h compiled over
oracle/ref_shims/, driven by oracle/ref_harness.cpp), built with plain numpy and small.

A scenario is a dict.  `script(sc)` turns it into the commands of the harness; `run_map(make, sc, ref)` runs it through
the common Python surface of oracle.OracleMap and binding.SdmMap (load_state / set_ring_state / set_stamps /
update(stop_after) and the read-backs); the `check_*` functions compare either with what the reference answered
(tests/golden/ref_ring_<variant>.npz, written by tests/golden/make_golden_ref_ring.py).

Two kinds.  exact: every float operation on the inputs gives one binary32 answer whatever the order of a sum
(positions on a voxel/8 lattice, weights in 1/64, axis-aligned paths, 90 degree object turns, one repeated noise value),
so everything is compared bit for bit.  random: seeded inputs; integers are compared exactly, floats within FLOAT_TOL,
and a point whose pixel or cell coordinate (recomputed in float64) lies within 1e-3 of an integer, or whose camera
depth lies within 1e-4 (relative) of a threshold it is tested against, is left out - at most 1 % of a scenario.
"""
import math

import numpy as np

from oracle import ref_ring
from semantic_dsp_map_amd import synth

F = np.float32
INVALID, UPDATED, REGULAR_BORN, GUESSED_BORN, COPIED, TIMEPTC = range(6)
IDENT_Q = np.array([1, 0, 0, 0], np.float32)
TURN_Q = np.array([0, 0, 1, 0], np.float32)          # half a turn about y: exact in binary32, unlike a quarter turn
NO_TRACK = 65535
STAGE_NO = {"ego": 1, "move": 2, "remove": 3, "visibility": 4, "weight": 5, "birth": 6, "occupancy": 7}
LP = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("sigma", "<f4"), ("track_id", "<u2"), ("label_id", "u1"), ("is_valid", "u1")])
OBJECT_MOVE = np.dtype([("track_id", "<i4"), ("T", "<f4", (16,))])
STATE = [("px", np.float32), ("py", np.float32), ("pz", np.float32), ("w", np.float32), ("ts", np.uint16),
         ("track", np.uint16), ("label", np.uint8), ("status", np.uint8), ("forget", np.uint8), ("owner", np.uint16)]

# Largest difference of a float output (wsum, a moved position) between two builds of the harness itself, -O0 and
# -O3 -march=native -ffp-contract=off (`make -C oracle ref-spread`, tests/golden/make_golden_ref_ring.py --spread):
# measured 0.0 in every random scenario of every variant.  The rule for a spread of 0 is one ulp of the largest
# magnitude in play: positions stay below 32 m (ulp 2^-19 in [16, 32)), weight sums below 8 (ulp 2^-21 in [4, 8)).
MEASURED_SPREAD = 0.0
FLOAT_TOL = {"pos": 2.0 ** -19, "wsum": 2.0 ** -21}
AMBIGUOUS_CAP = 0.01

# nb = 1 with the depth-noise flavour: a birth is one addNewParticleWithSemantics and draws no random number
PARAMS = dict(detection_probability=0.9, noise_number=0.05, nb_ptc_num_per_point=1, occupancy_threshold=0.25,
              max_obersevation_lost_time=5, forgetting_rate=1.0, max_forget_count=5, match_score_threshold=0.3,
              id_transition_probability=0.1, if_consider_depth_noise=1, if_use_independent_filter=0,
              depth_noise_first_order=0.0, depth_noise_zero_order=0.2)


def config(variant):
    return dict(synth.CONFIGS[ref_ring.VARIANTS[variant]])


def dims(cfg):
    return (1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]), 1 << cfg["p_n"]


# ------------------------------------------------------------------------------------------------ geometry
def ring_of(cfg, pos):
    """(moved steps, equivalent steps, map centre) after an ego update to pos, operations.h:1115-1122, 1196-1230"""
    n, _ = dims(cfg)
    vs = F(cfg["voxel_size"])
    recip = F(1) / vs
    steps = [int(F(F(pos[a]) * recip)) for a in range(3)]
    eq = [s % n[a] if s > 0 else -(-s % n[a]) for a, s in enumerate(steps)]
    return steps, eq, np.array([F(s) * vs for s in steps], F)


def cell_pos(cfg, pos, cell, frac=(0.5, 0.5, 0.5)):
    """global position at `frac` of map cell `cell` (map indices, 0 = the p_min side) of the ring centred for `pos`"""
    n, _ = dims(cfg)
    _, _, c = ring_of(cfg, pos)
    vs = float(F(cfg["voxel_size"]))
    return np.array([float(c[a]) - (n[a] >> 1) * vs + (cell[a] + frac[a]) * vs for a in range(3)], F)


def cell_coord(cfg, pos, p):
    """float64 map-cell coordinates of global points p for the ring centred for `pos` (for the ambiguity rule)"""
    n, _ = dims(cfg)
    _, _, c = ring_of(cfg, pos)
    vs = float(F(cfg["voxel_size"]))
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return np.stack([(p[:, a] - float(c[a]) + (n[a] >> 1) * vs) / vs for a in range(3)], 1)


def voxel_of(cfg, pos, p):
    """storage voxel of global point p in float32 as operations.h:849-900 computes it, None outside the map"""
    n, _ = dims(cfg)
    _, eq, c = ring_of(cfg, pos)
    vs = F(cfg["voxel_size"])
    recip = F(1) / vs
    r = []
    for a in range(3):
        pmin = -(F(n[a] >> 1) * vs)
        f = F(F(F(p[a]) - c[a]) - pmin) * recip
        if not (-1 < f < n[a]):
            return None
        i = int(f) + eq[a]
        r.append(i + n[a] if i < 0 else i - n[a] if i >= n[a] else i)
    return ((r[2] << cfg["y_n"]) | r[1]) << cfg["x_n"] | r[0]


def rotation(q):
    w, x, y, z = (float(v) for v in np.asarray(q, F))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def extrinsic(pos, q):
    """global -> camera, float64 then rounded: exact for IDENT_Q and TURN_Q, within an ulp or two of anyone's binary32
    evaluation otherwise (which is what the ambiguity rule of the random scenarios absorbs)"""
    r = rotation(q)
    e = np.eye(4)
    e[:3, :3] = r.T
    e[:3, 3] = -r.T @ np.asarray(pos, F).astype(np.float64)
    return e.astype(F)


def project(cfg, extr, p):
    """float64 (u, v, z) of global points"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    c = p @ extr[:3, :3].astype(np.float64).T + extr[:3, 3].astype(np.float64)
    z = c[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = cfg["fx"] * c[:, 0] / z + cfg["cx"]
        v = cfg["fy"] * c[:, 1] / z + cfg["cy"]
    return u, v, z, c


def near_int(x, eps=1e-3):
    return np.abs(x - np.round(x)) < eps


# ------------------------------------------------------------------------------------------------ state
class Sparse:
    """particles by slot index, in the order they were put"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.rows = {}

    def put(self, idx, pos=(0, 0, 0), w=0.0, ts=0, track=NO_TRACK, label=0, status=COPIED, forget=0, owner=NO_TRACK):
        assert idx not in self.rows, "slot %d used twice" % idx
        self.rows[int(idx)] = (F(pos[0]), F(pos[1]), F(pos[2]), F(w), int(ts), int(track), int(label), int(status), int(forget), int(owner))
        return int(idx)

    def free_slot(self, voxel):
        s = 1 << self.cfg["p_n"]
        for k in range(1, s):
            if voxel * s + k not in self.rows:
                return voxel * s + k
        return None

    def time_slot(self, voxel, ts):
        idx = voxel << self.cfg["p_n"]
        if idx not in self.rows:
            self.put(idx, ts=ts, track=0, status=TIMEPTC)

    def arrays(self):
        keys = ref_ring.STATE_KEYS + ("owner",)
        idx = sorted(self.rows)
        cols = list(zip(*[self.rows[i] for i in idx])) if idx else [[]] * 10
        out = {"idx": np.array(idx, np.int64)}
        for k, col in zip(keys[1:], cols):
            out[k] = np.array(col, np.float32 if k in ("px", "py", "pz", "w") else np.int64)
        return out


def empty_dense(cfg):
    n, s = dims(cfg)
    v = n[0] * n[1] * n[2]
    st = {k: np.zeros(v * s, dt) for k, dt in STATE}
    st["owner"][:] = NO_TRACK
    st["status"].reshape(v, s)[:, 0] = TIMEPTC
    return st


def dense(cfg, sp):
    st = empty_dense(cfg)
    for k, _ in STATE:
        if k in sp:
            st[k][sp["idx"]] = sp[k]
    return st


def sparse_of_dense(cfg, st):
    """the slots of a dense state that are not as clear() leaves them, as the harness dumps them"""
    _, s = dims(cfg)
    n = len(st["status"])
    cleared_status = np.where(np.arange(n) % s == 0, TIMEPTC, INVALID)
    dirty = st["status"] != cleared_status
    for k in ("px", "py", "pz", "w"):
        dirty |= st[k].view(np.uint32) != 0
    for k in ("ts", "track", "label", "forget"):
        dirty |= st[k] != 0
    idx = np.flatnonzero(dirty)
    out = {"idx": idx.astype(np.int64)}
    for k in ref_ring.STATE_KEYS[1:]:
        out[k] = st[k][idx].astype(np.float32 if k in ("px", "py", "pz", "w") else np.int64)
    return out


# ------------------------------------------------------------------------------------------------ scenarios
def _frame(name, variant, exact, path, pos, state, stop_after, q=IDENT_Q, moves=(), removes=(), depth=None, births=(),
           noise=(0.0,), fusion=None, fusion_voxels=(), **extra):
    cfg = config(variant)
    if depth is None:
        depth = np.zeros((cfg["height"], cfg["width"]), F)       # depth 0: the BFS bins nothing and stamps no voxel
    sc = dict(name=name, variant=variant, kind="frame", exact=exact, path=[np.asarray(p, F) for p in path], pos=np.asarray(pos, F),
              q=np.asarray(q, F), state=state.arrays(), stop_after=stop_after, moves=list(moves), removes=list(removes),
              depth=np.asarray(depth, F), births=list(births), noise=np.asarray(noise, F), fusion=fusion,
              fusion_voxels=list(fusion_voxels), ts=len(path) + 2)
    sc["extrinsic"] = extrinsic(sc["pos"], sc["q"])
    sc.update(extra)
    return sc


def lat(cfg, k):
    """k eighths of a voxel"""
    return F(F(k) * (F(cfg["voxel_size"]) / F(8)))


def ego_scenarios(variant):
    cfg = config(variant)
    n, _ = dims(cfg)
    q = min(n) >> 2                                  # the reference splits a move longer than q voxels, operations.h:71-90
    v = lambda k: float(lat(cfg, 8 * k))             # k voxels
    h = lambda k: float(lat(cfg, 8 * k + 4))         # k and a half voxels
    out = []
    # one axis at a time: short, a split jump, a jump of more than a whole ring (slabs recycled twice in one call),
    # then back through zero into the negative side
    a = [(h(3), 0, 0), (h(3) + v(q + 3), 0, 0), (h(3) + v(q + 3), -h(2), 0), (h(3) + v(q + 3), -h(2) - v(n[1] + 5), 0),
         (h(3) + v(q + 3), -h(2) - v(n[1] + 5), h(1)), (h(3) + v(q + 3), -h(2) - v(n[1] + 5), h(1)),
         (-h(4), -h(2) - v(n[1] + 5), h(1)), (-h(4), -h(2) - v(n[1] + 5), -h(2 * q + 1))]
    out.append(dict(name="ego_axes", variant=variant, kind="ego", exact=True, path=[np.array(p, F) for p in a]))
    # an equivalent step count of N - 1 on every axis, positive then negative; positions on whole voxels, where
    # pos * (1 / voxel) may fall a hair under the integer
    b, p = [], [0.0, 0.0, 0.0]
    for axis in range(3):
        for sign in (1, -1):
            target = sign * (n[axis] - 1)
            while round(p[axis] / v(1)) != target:
                cur = round(p[axis] / v(1))
                step = max(-q, min(q, target - cur))
                p[axis] = v(cur + step)
                b.append(tuple(p))
    out.append(dict(name="ego_wrap", variant=variant, kind="ego", exact=True, path=[np.array(p, F) for p in b]))
    rng = np.random.default_rng(101)
    c, p = [], np.zeros(3)
    for k in range(12):
        p = p + rng.uniform(-1, 1, 3) * np.array([n[0], n[1], n[2]]) * float(cfg["voxel_size"]) * (0.9 if k % 4 == 3 else 0.2)
        c.append(p.astype(F))
    out.append(dict(name="ego_random", variant=variant, kind="ego", exact=False, path=c))
    return out


def index_scenario(variant):
    cfg = config(variant)
    n, _ = dims(cfg)
    vs = float(F(cfg["voxel_size"]))
    pos = np.array([lat(cfg, 8 * 3 + 4), -lat(cfg, 8 * 2 + 4), 0], F)       # offsets +, -, 0
    _, _, c = ring_of(cfg, pos)
    half = np.array([(k >> 1) * vs for k in n])
    pts = [c - half.astype(F), c + half.astype(F), c.copy()]                 # exactly map_p_min, exactly map_p_max, the centre
    for a in range(3):
        lo, hi = c.copy(), c.copy()
        lo[a] = F(c[a] - F(half[a]))
        hi[a] = F(c[a] + F(half[a]))
        pts += [lo, hi]
    rng = np.random.default_rng(7)
    for _ in range(60):                                                      # the voxel/8 lattice, corners included
        k = rng.integers(-4 * np.array(n) - 8, 4 * np.array(n) + 8)
        pts.append(np.array([c[a] + lat(cfg, int(k[a])) for a in range(3)], F))
    exact_n = len(pts)
    for _ in range(300):
        pts.append((c + rng.uniform(-1, 1, 3) * (half + vs)).astype(F))
    pts = np.array(pts, F)
    amb = np.zeros(len(pts), bool)
    amb[exact_n:] = near_int(cell_coord(cfg, pos, pts[exact_n:])).any(1)
    return dict(name="index", variant=variant, kind="index", exact=False, path=[pos * F(0.5), pos], points=pts, ambiguous=amb)


def insert_scenario(variant):
    cfg = config(variant)
    n, s = dims(cfg)
    path = [np.array([lat(cfg, 28), 0, 0], F), np.array([lat(cfg, 28), -lat(cfg, 20), 0], F)]     # +3.5 voxels x (ts 1), -2.5 y (ts 2)
    pos = path[-1]
    ts = len(path) + 2
    st = Sparse(cfg)
    mid = [k >> 1 for k in n]
    cell = lambda dx, dy, dz: (mid[0] + dx, mid[1] + dy, mid[2] + dz)
    vox = lambda cl: voxel_of(cfg, pos, cell_pos(cfg, pos, cl))
    births, expect = [], []

    def fill(cl, slots, t=ts - 1, **kw):
        v = vox(cl)
        for k in slots:
            st.put(v * s + k, cell_pos(cfg, pos, cl, (0.25, 0.5, 0.75)), w=0.125, ts=t, label=1, **kw)
        return v

    def birth(cl, want_slot, label, frac=(0.5, 0.25, 0.5), track=NO_TRACK):
        births.append((cell_pos(cfg, pos, cl, frac), label, track))
        expect.append(None if want_slot is None else vox(cl) * s + want_slot)

    full = range(1, s)
    birth(cell(2, 1, 3), 1, 10)                                  # empty voxel
    birth(cell(2, 1, 3), 2, 11, track=40)                        # ... and the next slot, owned by an object
    fill(cell(-3, 2, 1), [1, 3])
    birth(cell(-3, 2, 1), 2, 12)                                 # partly filled: the first vacant slot, not the last
    birth(cell(-3, 2, 1), 4 if s > 4 else None, 13)              # ... then the next one, or full with 4 slots
    fill(cell(4, -2, -1), full)
    birth(cell(4, -2, -1), None, 14)                             # full
    fill((n[0] - 1, mid[1], mid[2] + 2), full, t=0)              # x slab recycled at ts 1: stamps older than it are stale
    birth((n[0] - 1, mid[1], mid[2] + 2), 1, 15)                 # full of stale slots
    fill((n[0] - 2, mid[1] + 1, mid[2] - 2), [1], t=0)
    fill((n[0] - 2, mid[1] + 1, mid[2] - 2), [2], t=1)
    birth((n[0] - 2, mid[1] + 1, mid[2] - 2), 1, 16)             # a point in a recycled slab: slot 1 stale, slot 2 (ts 1 = stamp) alive
    fill((mid[0], 0, mid[2] - 3), [1], t=1)                      # y slab recycled at ts 2: ts 1 is stale there
    birth((mid[0], 0, mid[2] - 3), 1, 17)
    v = fill(cell(-5, -3, 4), [k for k in full if k != 2])
    st.put(v * s + 2, cell_pos(cfg, pos, cell(-5, -3, 4)), w=0.25, ts=ts - 1, track=33, label=14, owner=33)
    birth(cell(-5, -3, 4), 2, 18)                                # removal of track 33, then insertion into its slot
    for corner, label in (((0, 0, 0), 19), (n, 20)):            # exactly on map_p_min (inside) and on map_p_max (outside)
        births.append((cell_pos(cfg, pos, corner, (0, 0, 0)), label, NO_TRACK))
        v = voxel_of(cfg, pos, births[-1][0])
        expect.append(None if v is None else v * s + 1)
    births.append((cell_pos(cfg, pos, (3 * n[0], mid[1], mid[2])), 21, NO_TRACK))    # far outside
    expect.append(None)
    # stopped after "birth", the frame also runs the WEIGHT stage, for which the harness has no counterpart: with the
    # all-zero depth image nothing is binned, so that stage touches no particle.  Give this scenario no depth.
    return _frame("insert", variant, True, path, pos, st, "birth", removes=[33], births=births, expect_slots=expect)


def guessed_add_scenario(variant):
    """addGuessedParticles (operations.h:192-205), which no stage of the frame reaches: the same slot choice, status
    GUESSED_BORN, the birth weight; into an empty voxel until it is full, beside live particles, and outside the map"""
    cfg = config(variant)
    n, s = dims(cfg)
    pos = np.array([-lat(cfg, 20), lat(cfg, 12), 0], F)
    mid = [k >> 1 for k in n]
    pts = [cell_pos(cfg, pos, (mid[0] + 1, mid[1], mid[2] - 2), (0.125 * (k % 8), 0.5, 0.25)) for k in range(s + 1)]
    pts += [cell_pos(cfg, pos, (0, 0, 0), (0, 0, 0)), cell_pos(cfg, pos, n, (0, 0, 0)), cell_pos(cfg, pos, (mid[0], 2 * n[1], mid[2]))]
    return dict(name="guessed_add", variant=variant, kind="adds", exact=True, path=[pos], points=np.array(pts, F), label=9, track=77, ts=3)


def _translation(t):
    m = np.eye(4, dtype=F)
    m[:3, 3] = t
    return m


def move_exact_scenario(variant):
    cfg = config(variant)
    n, s = dims(cfg)
    vs = float(F(cfg["voxel_size"]))
    path = [np.array([-lat(cfg, 12), 0, lat(cfg, 20)], F)]
    pos = path[-1]
    ts = len(path) + 2
    st = Sparse(cfg)
    mid = [k >> 1 for k in n]
    fr = (0.5, 0.375, 0.625)

    def obj(track, cells, label):
        for cl in cells:
            p = cell_pos(cfg, pos, cl, fr)
            st.put(st.free_slot(voxel_of(cfg, pos, p)), p, w=0.25, ts=ts - 1, track=track, label=label, status=UPDATED, owner=track)

    cells11 = [(mid[0] + dx, mid[1] + dy, mid[2] + dz) for dx, dy, dz in [(0, 0, 0), (1, 0, 0), (0, 1, 2), (3, -1, 1), (-2, 2, -3)]]
    obj(11, cells11, 14)
    t11 = np.array([lat(cfg, 16), 0, -lat(cfg, 9)], F)                        # +2 voxels x, -9/8 voxel z
    # object 12: a quarter turn about y, (x, y, z) -> (z, y, -x), then a translation that puts its first particle into the
    # voxel where object 11's first particle lands
    r = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)
    src12 = [cell_pos(cfg, pos, (mid[0] + dx, mid[1] + dy, mid[2] + dz), fr) for dx, dy, dz in [(-4, -2, 3), (-5, -2, 3), (-4, -3, 5)]]
    land = cell_pos(cfg, pos, cells11[0], fr).astype(np.float64) + t11 + np.array([lat(cfg, 1), 0, -lat(cfg, 1)])
    t12 = (land - r @ src12[0].astype(np.float64)).astype(F)
    for p in src12:
        st.put(st.free_slot(voxel_of(cfg, pos, p)), p, w=0.5, ts=ts - 1, track=12, label=15, status=UPDATED, owner=12)
    m12 = np.eye(4, dtype=F)
    m12[:3, :3] = r
    m12[:3, 3] = t12
    obj(13, [(mid[0] + 6, mid[1], mid[2] - 4), (mid[0] + 6, mid[1] + 1, mid[2] - 4)], 13)
    t13 = np.array([lat(cfg, 8 * n[0]), 0, 0], F)                             # a whole map to the side: out
    obj(14, [(mid[0] - 6, mid[1] - 4, mid[2] - 5)], 14)
    t14 = np.array([0, lat(cfg, 8), 0], F)                                    # one voxel up, into a voxel that is full
    vfull = voxel_of(cfg, pos, cell_pos(cfg, pos, (mid[0] - 6, mid[1] - 3, mid[2] - 5)))
    for k in range(1, s):
        st.put(vfull * s + k, cell_pos(cfg, pos, (mid[0] - 6, mid[1] - 3, mid[2] - 5)), w=0.125, ts=ts - 1, label=6)
    moves = [(11, _translation(t11)), (12, m12), (13, _translation(t13)), (99, _translation(t11)), (14, _translation(t14))]
    return _frame("move_exact", variant, True, path, pos, st, "move", moves=moves, noise=(2.0 ** -6,))


def move_overflow_scenario(variant):
    """The one place where the oracle knowingly departs from the reference: particles of ONE object that land in one
    voxel take its slots in the order the object's index set is walked - std::unordered_set order there, ascending index
    in the oracle (cpu_ref.cpp, PINNED at the owner sets) - and here more land than fit.

    Which of the object's particles win the slots is therefore not compared.  So that everything else can be, the
    object's particles differ in position only: weight, label and forget count are the same for all of them, and the
    multiset of the survivors' fields other than position does not depend on the walk order (check_frame asserts it
    in full).  A particle of no object already sits in the target voxel, with fields of its own; it keeps its slot."""
    cfg = config(variant)
    n, s = dims(cfg)
    path = [np.array([lat(cfg, 4), lat(cfg, 4), 0], F)]
    pos = path[-1]
    ts = len(path) + 2
    st = Sparse(cfg)
    mid = [k >> 1 for k in n]
    per = 1 if s <= 4 else 2
    for dx in (-1, 0):
        for dy in (-1, 0):
            for dz in (-1, 0):
                for j in range(per):                 # near the corner the eight voxels share
                    fr = tuple(0.875 - 0.125 * j if d < 0 else 0.125 + 0.125 * j for d in (dx, dy, dz))
                    p = cell_pos(cfg, pos, (mid[0] + dx, mid[1] + dy, mid[2] + dz), fr)
                    st.put(st.free_slot(voxel_of(cfg, pos, p)), p, w=0.140625, ts=ts - 1, track=21, label=14, status=UPDATED, forget=1, owner=21)
    p = cell_pos(cfg, pos, mid, (0.75, 0.25, 0.5))
    st.put(st.free_slot(voxel_of(cfg, pos, p)), p, w=0.25, ts=ts - 1, label=6, status=UPDATED, forget=2)
    t = np.array([lat(cfg, 4), lat(cfg, 4), lat(cfg, 4)], F)    # half a voxel: all of them land in cell `mid`
    return _frame("move_overflow", variant, True, path, pos, st, "move", moves=[(21, _translation(t))], noise=(0.0,),
                  target_voxel=voxel_of(cfg, pos, p))


def move_random_scenario(variant):
    cfg = config(variant)
    n, s = dims(cfg)
    vs = float(F(cfg["voxel_size"]))
    rng = np.random.default_rng(31)
    path = [(rng.uniform(-3, 3, 3) * vs).astype(F)]
    pos = path[-1]
    ts = len(path) + 2
    st = Sparse(cfg)
    noise = F(rng.normal(0, 0.05))
    moves = []
    for track in (5, 6, 7):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-0.5, 0.5)
        kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        r = np.eye(3) + math.sin(ang) * kx + (1 - math.cos(ang)) * kx @ kx
        m = np.eye(4)
        m[:3, :3] = r
        centre = cell_pos(cfg, pos, [k >> 1 for k in n]).astype(np.float64)
        m[:3, 3] = centre - r @ centre + rng.uniform(-2, 2, 3) * vs
        m = m.astype(F)
        seen = set()
        for _ in range(40):
            p = (centre + rng.uniform(-0.3, 0.3, 3) * np.array(n) * vs).astype(F)
            v = voxel_of(cfg, pos, p)
            q = m[:3, :3].astype(np.float64) @ p.astype(np.float64) + m[:3, 3] + float(noise)
            cc = cell_coord(cfg, pos, q)[0]
            key = tuple(np.floor(cc).astype(int))
            # left out at build time: a target within 1e-3 of a cell border, and a second particle of the same object
            # in one target voxel (their slots would follow the walk order of the object's set)
            if v is None or near_int(cc).any() or key in seen or st.free_slot(v) is None:
                continue
            seen.add(key)
            st.put(st.free_slot(v), p, w=F(rng.uniform(0.05, 0.9)), ts=ts - 1, track=track, label=13 + track % 3, status=UPDATED, owner=track)
        moves.append((track, m))
    return _frame("move_random", variant, False, path, pos, st, "move", moves=moves, noise=(noise,))


def _depth_image(cfg, scale=1.0):
    """0 (nothing is seen) but for a window round the principal point: 5 m, with a band beyond the range, a band of NaN,
    a band of 0 and a near patch of 2 m that hides what is behind it"""
    h, w = cfg["height"], cfg["width"]
    d = np.zeros((h, w), F)
    hh, hw = int(h * 0.3 * scale), int(w * 0.3 * scale)
    r0, c0 = int(cfg["cy"]) - hh, int(cfg["cx"]) - hw
    win = d[r0:r0 + 2 * hh, c0:c0 + 2 * hw]
    win[:] = 5.0
    win[:, :hw // 2] = cfg["depth_max"] + 5.0
    win[:hh // 3, :] = np.nan
    win[-(hh // 3):, :] = 0.0
    win[hh // 2:hh, hw:hw + hw // 2] = 2.0
    return d


def _visible(name, variant, exact, q, seed, n_particles, scale):
    cfg = config(variant)
    n, s = dims(cfg)
    vs = float(F(cfg["voxel_size"]))
    rng = np.random.default_rng(seed)
    path = [np.array([lat(cfg, 20), 0, -lat(cfg, 12)], F), np.array([lat(cfg, 20), lat(cfg, 12), -lat(cfg, 12)], F)]
    pos = path[-1]
    ts = len(path) + 2
    depth = _depth_image(cfg, scale)
    extr = extrinsic(pos, q)
    r = rotation(q)
    st = Sparse(cfg)
    hh, hw = int(cfg["height"] * 0.3 * scale), int(cfg["width"] * 0.3 * scale)
    reach = min(min(n) * vs / 2 - vs, 8.0)
    tries = 0
    while len(st.rows) < n_particles and tries < 50 * n_particles:
        tries += 1
        z = rng.uniform(0.2, reach)
        cam = np.array([rng.uniform(-1.3, 1.3) * hw * z / cfg["fx"], rng.uniform(-1.3, 1.3) * hh * z / cfg["fy"], z])
        p = r @ cam + pos.astype(np.float64)
        if exact:
            p = np.array([pos[a] + lat(cfg, int(round((p[a] - float(pos[a])) / (vs / 8)))) for a in range(3)], F)
        p = p.astype(F)
        v = voxel_of(cfg, pos, p)
        if v is None or st.free_slot(v) is None:
            continue
        w = F(rng.integers(1, 64) / 64.0) if exact else F(rng.uniform(0.01, 1.2))
        stale = rng.random() < 0.05
        st.put(st.free_slot(v), p, w=w, ts=0 if stale else ts - 1, track=int(rng.choice([NO_TRACK, 3, 4])), label=int(rng.integers(0, 16)),
               status=int(rng.choice([UPDATED, REGULAR_BORN, GUESSED_BORN, COPIED])), forget=int(rng.integers(0, 3)))
    sc = _frame(name, variant, exact, path, pos, st, "visibility", q=q, depth=depth)
    sp = sc["state"]
    pts = np.stack([sp["px"], sp["py"], sp["pz"]], 1)
    u, v, z, _ = project(cfg, extr, pts)
    amb = near_int(u) | near_int(v)                 # the voxel of a loaded particle is its slot's: no cell coordinate decides here
    row, col = np.clip(np.floor(v), 0, cfg["height"] - 1).astype(int), np.clip(np.floor(u), 0, cfg["width"] - 1).astype(int)
    d = depth[row, col].astype(np.float64)
    for thr in (np.full(len(z), cfg["depth_min"]), np.full(len(z), cfg["depth_max"]), d * 1.1, d):
        with np.errstate(invalid="ignore"):
            amb |= np.abs(z - thr) <= 1e-4 * np.abs(thr)
    if exact:                                       # an exact scenario leaves nothing out, points on cell borders included
        amb[:] = False
    sc["ambiguous_idx"] = sp["idx"][amb & (sp["status"] != TIMEPTC)]
    sc["n_points"] = int((sp["status"] != TIMEPTC).sum())
    # the BFS start vertex, one metre down the optical axis, must not sit on a cell border either
    start = cell_coord(cfg, pos, (r @ np.array([0, 0, 1.0]) + pos.astype(np.float64)))[0]
    assert exact or not near_int(start, 1e-2).any(), "move the camera: its BFS start vertex is on a cell border"
    return sc


# seeds for which the ambiguous share of the oblique view stays under AMBIGUOUS_CAP (13 gives 5 of 400 points in t0)
OBLIQUE_SEED = {"zed2_boost": 13, "t1": 13, "t0": 14}


def _oblique_q(yaw_deg, pitch_deg=-11.0):
    yaw, pitch = math.radians(yaw_deg), math.radians(pitch_deg)
    qy = np.array([math.cos(yaw / 2), 0, math.sin(yaw / 2), 0])
    qx = np.array([math.cos(pitch / 2), math.sin(pitch / 2), 0, 0])
    return np.array([qy[0] * qx[0], qy[0] * qx[1], qy[2] * qx[0], -qy[2] * qx[1]], F)   # the product qy * qx


# The BFS starts at the vertex below the point one metre down the optical axis (operations.h:1312-1321); with big
# voxels and a turned camera that vertex can lie outside the frustum, and then the reference sees nothing at all
# (t0 at 33 degrees).  The oblique view is to bin particles, so each variant gets a yaw at which it does.
OBLIQUE_YAW = {"zed2_boost": 33.0, "t1": 33.0, "t0": 42.0}


def visible_scenarios(variant):
    scale = 0.35 if variant == "zed2_boost" else 1.0
    q = _oblique_q(OBLIQUE_YAW[variant])
    return [_visible("visible_z", variant, True, IDENT_Q, 11, 260, scale),
            _visible("visible_back", variant, True, TURN_Q, 12, 120, scale),
            _visible("visible_oblique", variant, False, q, OBLIQUE_SEED[variant], 400, scale)]


def _fusion_state(cfg, pos, ts, exact, seed):
    n, s = dims(cfg)
    rng = np.random.default_rng(seed)
    st = Sparse(cfg)
    mid = [k >> 1 for k in n]
    used = []

    def voxel(cl, stamp=ts - 1):
        v = voxel_of(cfg, pos, cell_pos(cfg, pos, cl))
        st.time_slot(v, stamp)
        used.append(v)
        return v

    def put(v, k, w, status=UPDATED, track=NO_TRACK, label=0, t=ts - 1):
        st.put(v * s + k, (0, 0, 0), w=w, ts=t, track=track, label=label, status=status)

    if exact:
        v = voxel((mid[0] + 1, mid[1], mid[2]))                 # two tracks of equal weight: the lower id wins (strict >)
        put(v, 1, 0.25, track=9, label=3)
        put(v, 2, 0.25, track=5, label=2)
        v = voxel((mid[0] + 2, mid[1], mid[2]))                 # guessed only, enough for "guessed occupied"
        put(v, 1, 0.0625, status=GUESSED_BORN, track=8, label=4)
        v = voxel((mid[0] + 2, mid[1] + 2, mid[2]))             # guessed only, exactly the birth weight 0.05f: still >= it
        put(v, 1, F(0.05), status=GUESSED_BORN, track=8, label=4)
        v = voxel((mid[0] + 3, mid[1], mid[2]))                 # guessed only, too light
        put(v, 2, 0.03125, status=GUESSED_BORN, track=8, label=4)
        v = voxel((mid[0] + 4, mid[1], mid[2]))                 # exactly at the threshold 0.25: not occupied
        put(v, 1, 0.125, track=6, label=5)
        put(v, 3, 0.125, track=6, label=5)
        v = voxel((mid[0] + 5, mid[1], mid[2]))                 # 1/64 above it
        put(v, 1, 0.125, track=6, label=5)
        put(v, 2, 0.140625, track=7, label=6)
        v = voxel((mid[0] + 1, mid[1] + 1, mid[2]))             # a weight above 1: summed as it is, then clamped
        put(v, 1, 1.5, status=COPIED, track=2, label=7)
        v = voxel((mid[0] + 2, mid[1] + 1, mid[2]))             # a light UPDATED particle: summed, then deleted, no vote
        put(v, 1, 0.03125, track=1, label=9)
        put(v, 2, 0.046875, status=REGULAR_BORN, track=2, label=10)
        v = voxel((mid[0] + 3, mid[1] + 1, mid[2]))             # stale particles beside a live one
        put(v, 1, 0.5, track=3, label=11, t=0)
        put(v, 2, 0.125, track=4, label=12)
        v = voxel((n[0] - 1, mid[1] + 1, mid[2]), stamp=0)      # never observed: unknown whatever it holds
        put(v, 1, 0.5, track=3, label=11)
        v = voxel((n[0] - 1, mid[1] + 2, mid[2]), stamp=ts - 1)  # in the recycled x slab (stamp 1): alive, ts 0 would be stale
        put(v, 1, 0.5, track=3, label=11, t=0)
        put(v, 2, 0.375, track=4, label=12, t=1)
        v = voxel((mid[0] + 4, mid[1] + 1, mid[2]))             # every slot taken, three tracks
        for k in range(1, s):
            put(v, k, 0.0625 * (1 + k % 3), track=20 + k % 3, label=1 + k % 3, status=[UPDATED, COPIED, REGULAR_BORN][k % 3])
        v = voxel((mid[0] + 5, mid[1] + 1, mid[2]))             # observed and empty: free
    else:
        for _ in range(220):
            cl = [int(rng.integers(0, k)) for k in n]
            v = voxel_of(cfg, pos, cell_pos(cfg, pos, cl))
            if v in used:
                continue
            voxel(cl, stamp=int(rng.choice([ts - 1, ts - 1, ts - 1, 0])))
            fill = float(rng.choice([0.6, 0.6, 1.5 / s]))           # some voxels hold one or two particles only
            for k in range(1, s):
                if rng.random() < fill:
                    put(v, k, F(rng.uniform(0.0, 0.6) if rng.random() < 0.9 else rng.uniform(0.9, 1.6)),
                        status=int(rng.choice([UPDATED, UPDATED, REGULAR_BORN, GUESSED_BORN, COPIED])),
                        track=int(rng.choice([NO_TRACK, 1, 2, 3])), label=int(rng.integers(0, 16)), t=int(rng.choice([ts - 1, ts - 1, ts - 1, 0])))
    return st, used


def fusion_scenarios(variant):
    cfg = config(variant)
    path = [np.array([lat(cfg, 12), 0, 0], F)]                  # 1.5 voxels: the x slab at the far side is recycled at ts 1
    pos = path[-1]
    ts = len(path) + 2
    out = []
    for exact, seed in ((True, 0), (False, 55)):
        tag = "exact" if exact else "random"
        st, used = _fusion_state(cfg, pos, ts, exact, seed)
        out.append(_frame("occupancy_" + tag, variant, exact, path, pos, st, "occupancy"))
        st, used = _fusion_state(cfg, pos, ts, exact, seed)
        out.append(_frame("wsum_" + tag, variant, exact, path, pos, st, "occupancy", fusion="plain", fusion_voxels=used))
    return out


def neighbours_scenario(variant):
    """calculateWeightAndSemanticsInVoxelConsiderNeighbors (operations.h:457-600): a centre voxel on every face of the map
    and at every ring index where the unwrapped neighbour tests change (0, 1, 2, N - 3, N - 2, N - 1)"""
    cfg = config(variant)
    n, s = dims(cfg)
    path = [np.array([lat(cfg, 8 * 5 + 4), -lat(cfg, 8 * 3 + 4), lat(cfg, 12)], F)]
    pos = path[-1]
    ts = len(path) + 2
    _, eq, _ = ring_of(cfg, pos)
    rng = np.random.default_rng(77)
    st = Sparse(cfg)
    mid = [k >> 1 for k in n]
    centres = []
    cells = []
    for a in range(3):                                           # the six faces of the map
        for side in (0, n[a] - 1):
            cl = list(mid)
            cl[a] = side
            cl[(a + 1) % 3] += 3 * a + (1 if side else -2)
            cells.append(tuple(cl))
    for a in (0, 1):                                             # the ring-index edges of x and y
        for ring_i in (0, 1, 2, n[a] - 3, n[a] - 2, n[a] - 1):
            cl = [mid[0] - 5, mid[1] - 5, mid[2] + 4 + 2 * a]
            cl[a] = (ring_i - eq[a]) % n[a]
            cl[1 - a] += ring_i % 7
            cells.append(tuple(cl))
    for k in range(24):
        cells.append(tuple(int(rng.integers(2, d - 2)) for d in n))
    weights = [0.0, 0.125, 0.25, 0.5, 0.375]
    lonely = set(cells[-6:])                                     # heavy centres whose neighbours hold nothing: "all empty"
    hollow = set(cells[-12:-6])                                  # empty centres between heavy neighbours: the inferred weight
    for cl in cells:
        vc = voxel_of(cfg, pos, cell_pos(cfg, pos, cl))
        if vc in centres:
            continue
        centres.append(vc)
        for d in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            c2 = (cl[0] + d[0], cl[1] + d[1], cl[2])
            if not (0 <= c2[0] < n[0] and 0 <= c2[1] < n[1]):
                continue
            v = voxel_of(cfg, pos, cell_pos(cfg, pos, c2))
            if (v << cfg["p_n"]) in st.rows:
                continue
            st.time_slot(v, int(rng.choice([ts - 1, ts - 1, ts - 1, ts - 1, 0])))
            for k in range(1, s):
                w = float(rng.choice(weights))
                if cl in lonely:
                    w = 0.5 if d == (0, 0) and k == 1 else 0.0
                elif cl in hollow:
                    w = 0.0 if d == (0, 0) else 0.5 if k == 1 else 0.0
                if w:
                    st.put(v * s + k, (0, 0, 0), w=w if rng.random() < 0.9 else 1.25, ts=ts - 1, track=int(rng.choice([1, 2, 3])), label=int(rng.integers(1, 9)),
                           status=int(rng.choice([UPDATED, UPDATED, REGULAR_BORN, GUESSED_BORN, COPIED])))
                elif rng.random() < 0.2:
                    st.put(v * s + k, (0, 0, 0), w=0.03125, ts=ts - 1, track=4, label=9, status=UPDATED)
    # as in insert_scenario: "birth" runs the WEIGHT stage too, which the harness lacks; the all-zero depth bins nothing
    return _frame("neighbours", variant, True, path, pos, st, "birth", fusion="neighbours", fusion_voxels=centres)


def frustum_scenario(variant):
    cfg = config(variant)
    vs = float(F(cfg["voxel_size"]))
    rng = np.random.default_rng(91)
    yaw = math.radians(-41.0)
    q = np.array([math.cos(yaw / 2), 0, math.sin(yaw / 2), 0], F)
    pos = np.array([lat(cfg, 9), -lat(cfg, 3), lat(cfg, 14)], F)
    extr = extrinsic(pos, q)
    r = rotation(q)
    tx, ty = cfg["width"] / 2.0 / cfg["fx"], cfg["height"] / 2.0 / cfg["fy"]
    pts = []
    for _ in range(400):
        z = rng.choice([rng.uniform(0.0, 1.0), rng.uniform(1.0, cfg["depth_max"] + 2.0)])
        pts.append(r @ np.array([rng.uniform(-1.4, 1.4) * tx * z, rng.uniform(-1.4, 1.4) * ty * z, z]) + pos)
    pts = np.array(pts, F)
    _, _, z, c = project(cfg, extr, pts)
    amb = np.zeros(len(pts), bool)
    for thr in (cfg["depth_min"], cfg["depth_max"]):
        amb |= np.abs(z - thr) <= 1e-4 * thr
    amb |= np.abs(np.abs(c[:, 0]) - z * tx) <= 1e-4 * np.abs(z * tx)
    amb |= np.abs(np.abs(c[:, 1]) - z * ty) <= 1e-4 * np.abs(z * ty)
    # exact: the camera looks along +z from a lattice point; lattice points, with the planes z = depth_min / depth_max
    # and x = +- z tan (half fov) among them where the lattice meets them
    epos = np.array([lat(cfg, 8), 0, -lat(cfg, 16)], F)
    epts = []
    for _ in range(200):
        z = rng.choice([rng.uniform(0.0, 1.0), rng.uniform(1.0, cfg["depth_max"] + 2.0)])
        cam = np.array([rng.uniform(-1.4, 1.4) * tx * z, rng.uniform(-1.4, 1.4) * ty * z, z])
        epts.append(np.array([epos[a] + lat(cfg, int(round(cam[a] / (vs / 8)))) for a in range(3)], F))
    for kz in (1, 2, 3):                                         # on the planes x = +- z tan, y = +- z tan themselves
        for sx in (-1, 1):
            zz = float(lat(cfg, 16 * kz))
            epts.append(np.array([epos[0] + F(sx * zz * tx), epos[1], epos[2] + F(zz)], F))
            epts.append(np.array([epos[0], epos[1] + F(sx * zz * ty), epos[2] + F(zz)], F))
    return dict(name="frustum", variant=variant, kind="frustum", exact=False,
                views=[dict(pos=epos, q=IDENT_Q, extrinsic=extrinsic(epos, IDENT_Q), points=np.array(epts, F), ambiguous=np.zeros(len(epts), bool)),
                       dict(pos=pos, q=q, extrinsic=extr, points=pts, ambiguous=amb)])


def tables_scenario(variant):
    rng = np.random.default_rng(3)
    t = []
    for _ in range(300):
        mu, sigma = rng.uniform(-5, 5), rng.uniform(0.05, 0.6)
        t.append((mu + rng.uniform(-12, 12) * sigma, mu, sigma))
    t += [(9.9, 0.0, 1.0), (-9.9, 0.0, 1.0), (9.95, 0.0, 1.0), (-9.95, 0.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 1.0), (0.0, 0.5, 0.25)]
    return dict(name="tables", variant=variant, kind="tables", exact=True, queries=np.array(t, F), forgetting=(F(PARAMS["forgetting_rate"]),
                PARAMS["max_forget_count"], [0, 1, 2, 3, 4, 5, 7]))


def bfs_limits_scenario(variant):
    """What the reference's BFS cannot be asked: a start vertex outside the vertex grid (it indexes unchecked), which
    for the multi-threaded form is every view of these variants (its threads start at depth_max / 1.26 and depth_max,
    beyond half the map)."""
    cfg = config(variant)
    n, _ = dims(cfg)
    pos = np.array([lat(cfg, 4), 0, 0], F)
    far = pos + np.array([0, 0, lat(cfg, 8 * n[2])], F)
    return dict(name="bfs_limits", variant=variant, kind="bfs_limits", exact=True, pos=pos,
                views=[(extrinsic(far, IDENT_Q), False), (extrinsic(pos, IDENT_Q), True), (extrinsic(pos, IDENT_Q), False)])


def scenarios(variant):
    out = ego_scenarios(variant) + [index_scenario(variant), insert_scenario(variant), guessed_add_scenario(variant), move_exact_scenario(variant),
                                    move_overflow_scenario(variant), move_random_scenario(variant)]
    out += visible_scenarios(variant) + fusion_scenarios(variant) + [neighbours_scenario(variant), frustum_scenario(variant),
                                                                    bfs_limits_scenario(variant)]
    if variant == "t1":
        out.append(tables_scenario(variant))
    return out


# ------------------------------------------------------------------------------------------------ harness scripts
def birth_pixels(cfg, k):
    """pixel of the k-th birth: the first pass of the birth raster (semantic_dsp_map.h:778-800) visits rows and columns
    0, 3, 6, ... in row-major order"""
    per_row = (cfg["width"] + 2) // 3
    return 3 * (k // per_row), 3 * (k % per_row)


def script(sc):
    cfg = config(sc["variant"])
    s = ref_ring.Script()
    kind = sc["kind"]
    if kind == "ego":
        for t, p in enumerate(sc["path"], 1):
            s.ts(t)
            s.ego(p)
            s.dump("ring", "stamps")
    elif kind == "index":
        for t, p in enumerate(sc["path"], 1):
            s.ts(t)
            s.ego(p)
        s.dump("ring", "stamps")
        s.pos_to_voxel(sc["points"])
    elif kind == "adds":
        s.ts(1)
        s.ego(sc["path"][0])
        s.dump("ring")
        s.ts(sc["ts"])
        s.add(sc["points"], sc["label"], sc["track"], guessed=True)
        s.dump("state")
    elif kind == "tables":
        s.pdf_table()
        s.query_pdf(sc["queries"])
        s.forgetting_factor(*sc["forgetting"])
    elif kind == "frustum":
        for view in sc["views"]:
            s.frustum(view["extrinsic"], view["points"])
    elif kind == "bfs_limits":
        s.ts(1)
        s.ego(sc["pos"])
        depth = np.zeros((cfg["height"], cfg["width"]), F)
        for extr, mt in sc["views"]:
            s.visible(extr, depth, multi_threaded=mt)
    else:
        stage = STAGE_NO[sc["stop_after"]]
        sp = sc["state"]
        s.noise(sc["noise"])
        for t, p in enumerate(sc["path"], 1):
            s.ts(t)
            s.ego(p)
        s.dump("ring", "stamps")
        s.load(sp)
        s.ts(sc["ts"])
        s.ego(sc["pos"])
        if stage >= 2:
            sets = [(sp["idx"][sp["owner"] == track], m) for track, m in sc["moves"]]
            sets = [(i, m) for i, m in sets if len(i)]                      # checkIfObjectExists, semantic_dsp_map.h:611
            if sets:
                s.move([i for i, _ in sets], [m for _, m in sets])
        if stage >= 3:
            for track in sc["removes"]:
                s.delete(sp["idx"][sp["owner"] == track])
        if stage >= 4:
            s.visible(sc["extrinsic"], sc["depth"])
        if stage >= 6:
            for p, label, track in sc["births"]:
                s.add([p], label, track)
        if sc["fusion"]:
            s.fusion(sc["fusion_voxels"], PARAMS["occupancy_threshold"], neighbours=sc["fusion"] == "neighbours")
        elif stage >= 7:
            s.occupancy(PARAMS["occupancy_threshold"])
        s.dump("ring", "stamps", "state", "bins")
    return s.text()


def index_script_tail(sc, voxels):
    """second run of an index scenario: the same ring, then voxel -> position for the voxels the first run found"""
    s = ref_ring.Script()
    for t, p in enumerate(sc["path"], 1):
        s.ts(t)
        s.ego(p)
    s.voxel_to_pos(voxels)
    return s.text()


# ------------------------------------------------------------------------------------------------ running a map
def ring_dict(ref_ring_rec, gts):
    return {"global_time_stamp": gts, "moved_steps": list(ref_ring_rec["moved_steps"]), "eq_steps": list(ref_ring_rec["eq_steps"]),
            "map_center": [float(x) for x in ref_ring_rec["map_center"]], "last_pos": [float(x) for x in ref_ring_rec["last_pos"]],
            "birth_cursor": 0, "move_cursor": 0}


def noise_table(sc):
    return np.resize(np.asarray(sc.get("noise", [0.0]), F), 1000000)


def blank(cfg):
    return np.zeros(cfg["width"] * cfg["height"], F), np.zeros(cfg["width"] * cfg["height"], LP)


def make_map(make, sc, bin_order=0):
    cfg = config(sc["variant"])
    return make(dict(cfg, bin_order=bin_order), PARAMS, noise_table(sc))


def split_bins(m):
    counts = m.bin_counts().reshape(-1)
    flat = m.bins()
    out, at = {}, 0
    for pid in np.flatnonzero(counts):
        out[int(pid)] = flat[at:at + counts[pid]].copy()
        at += int(counts[pid])
    return out


def run_ego(make, sc):
    """every step of the path as a frame stopped after the ego stage; -> [(ring, stamps)] per step"""
    cfg = config(sc["variant"])
    m = make_map(make, sc)
    depth, cloud = blank(cfg)
    out = []
    for p in sc["path"]:
        m.update(depth, cloud, p, IDENT_Q, stop_after="ego")
        out.append((m.ring_state(), m.stamps()))
    return out


def run_frame(make, sc, records):
    """the frame of a scenario on a map put into the state the reference was in before it"""
    cfg = config(sc["variant"])
    m = make_map(make, sc)
    m.load_state(dense(cfg, sc["state"]))
    m.set_ring_state(ring_dict(ref_ring.first(records, "ring", 0), sc["ts"] - 1))
    m.set_stamps(*ref_ring.first(records, "stamps", 0))
    depth, cloud = sc["depth"].reshape(-1), blank(cfg)[1]
    for k, (p, label, track) in enumerate(sc["births"]):
        r, c = birth_pixels(cfg, k)
        pt = cloud[r * cfg["width"] + c:r * cfg["width"] + c + 1]
        pt["x"], pt["y"], pt["z"] = p
        pt["sigma"], pt["track_id"], pt["label_id"], pt["is_valid"] = 0.2, track, label, 1
    moves = np.zeros(len(sc["moves"]), OBJECT_MOVE)
    for k, (track, mat) in enumerate(sc["moves"]):
        moves[k]["track_id"] = track
        moves[k]["T"] = np.asarray(mat, F).reshape(-1)
    m.update(depth, cloud, sc["pos"], sc["q"], moves, sc["removes"], stop_after=sc["stop_after"])
    return m


# ------------------------------------------------------------------------------------------------ comparisons
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_ring(ref, got, what):
    assert got["global_time_stamp"] == ref["global_time_stamp"], what
    assert list(got["moved_steps"]) == list(ref["moved_steps"]), (what, got["moved_steps"], ref["moved_steps"])
    assert list(got["eq_steps"]) == list(ref["eq_steps"]), (what, got["eq_steps"], ref["eq_steps"])
    assert np.array_equal(bits(got["map_center"]), bits(ref["map_center"])), (what, got["map_center"], ref["map_center"])
    assert np.array_equal(bits(got["last_pos"]), bits(ref["last_pos"])), what


def check_stamps(ref, got, what):
    for a, (r, g) in enumerate(zip(ref, got)):
        assert np.array_equal(np.asarray(r, np.int64), np.asarray(g, np.int64)), "%s: time stamps of axis %d differ at %s" % (
            what, a, np.flatnonzero(np.asarray(r, np.int64) != np.asarray(g, np.int64))[:8])


def check_state(sc, ref_sp, got_dense, what, skip_idx=(), live_only=False, pos_tol=None, skip_voxels=()):
    """ref_sp: the harness's dump; got_dense: dump_state() of the map.  Every field of every slot, bit for bit - or, with
    live_only, the status of every slot and the fields of the slots that are not INVALID (for a map that does not keep
    what a deleted particle leaves behind)."""
    cfg = config(sc["variant"])
    _, s = dims(cfg)
    ref = dense(cfg, ref_sp)
    keep = np.ones(len(ref["status"]), bool)
    keep[np.asarray(list(skip_idx), np.int64)] = False
    for v in skip_voxels:
        keep[v * s:(v + 1) * s] = False
    assert np.array_equal(ref["status"][keep], got_dense["status"][keep]), "%s: status differs at slots %s" % (
        what, np.flatnonzero(keep & (ref["status"] != got_dense["status"]))[:8])
    if live_only:
        keep &= ref["status"] != INVALID
    for k in ("ts", "track", "label", "forget"):
        bad = keep & (ref[k] != got_dense[k])
        assert not bad.any(), "%s: %s differs at slots %s: reference %s, got %s" % (what, k, np.flatnonzero(bad)[:8], ref[k][bad][:8], got_dense[k][bad][:8])
    for k in ("px", "py", "pz", "w"):
        if pos_tol is not None and k != "w":
            bad = keep & ~(np.abs(ref[k].astype(np.float64) - got_dense[k].astype(np.float64)) <= pos_tol)
        else:
            bad = keep & (bits(ref[k]) != bits(got_dense[k]))
        assert not bad.any(), "%s: %s differs at slots %s: reference %s, got %s" % (what, k, np.flatnonzero(bad)[:8], ref[k][bad][:8], got_dense[k][bad][:8])


def check_bins(ref_bins, got_bins, what, ordered, skip_idx=()):
    skip = set(int(i) for i in skip_idx)
    f = lambda b: {p: [int(i) for i in v if int(i) not in skip] for p, v in b.items()}
    r = {p: v for p, v in f(ref_bins).items() if v}
    g = {p: v for p, v in f(got_bins).items() if v}
    assert sorted(r) == sorted(g), "%s: pixels with particles differ: %s" % (what, sorted(set(r) ^ set(g))[:8])
    for p in r:
        if ordered:
            assert r[p] == g[p], "%s: pixel %d holds %s, reference %s" % (what, p, g[p], r[p])
        else:
            assert sorted(r[p]) == sorted(g[p]), "%s: pixel %d holds %s, reference %s" % (what, p, g[p], r[p])


def check_occupancy(sc, occ_rec, voxels, what):
    cfg = config(sc["variant"])
    n, _ = dims(cfg)
    v = n[0] * n[1] * n[2]
    occ = np.full(v, -1, np.int64)
    label, track = np.zeros(v, np.int64), np.zeros(v, np.int64)
    rows = occ_rec["rows"]
    occ[rows[:, 0]], label[rows[:, 0]], track[rows[:, 0]] = rows[:, 1], rows[:, 2], rows[:, 3]
    assert occ_rec["unknown"] + len(rows) == v
    for k, r in (("occ", occ), ("label", label), ("track", track)):
        bad = np.flatnonzero(voxels[k].astype(np.int64) != r)
        assert not len(bad), "%s: %s differs at voxels %s: reference %s, got %s" % (what, k, bad[:8], r[bad][:8], voxels[k][bad][:8])


def check_wsum(sc, fus, got_wsum, what):
    ref = fus["wsum"]
    if sc["exact"]:
        bad = np.flatnonzero(bits(ref) != bits(got_wsum))
    else:
        bad = np.flatnonzero(~(np.abs(ref.astype(np.float64) - got_wsum.astype(np.float64)) <= FLOAT_TOL["wsum"]))
    assert not len(bad), "%s: wsum differs at %s: reference %s, got %s" % (what, bad[:8], ref[bad][:8], got_wsum[bad][:8])


def ambiguous_share(sc):
    if sc["kind"] == "index":
        return float(sc["ambiguous"].mean())
    if sc["kind"] == "frustum":
        return max(float(v["ambiguous"].mean()) for v in sc["views"])
    if "ambiguous_idx" in sc:
        return len(sc["ambiguous_idx"]) / max(sc["n_points"], 1)
    return 0.0


def survivors(cfg, st, voxel):
    """multiset of (w, ts, track, label, status, forget) of the live slots of a voxel"""
    s = dims(cfg)[1]
    rows = []
    for i in range(voxel * s + 1, (voxel + 1) * s):
        if st["status"][i] != INVALID:
            rows.append((int(bits(st["w"][i:i + 1])[0]), int(st["ts"][i]), int(st["track"][i]), int(st["label"][i]), int(st["status"][i]), int(st["forget"][i])))
    return sorted(rows)


def check_frame(sc, rec, m, bins_ordered):
    """a map after the frame of a scenario (run_frame) against the reference's answer `rec` (ref_ring.parse of the fixture).
    bins_ordered: the per-pixel lists in the reference's push order (the oracle with bin_order=0); otherwise in ascending
    index order, the canonical order of the HIP library."""
    cfg, name = config(sc["variant"]), sc["name"]
    s = dims(cfg)[1]
    check_ring(ref_ring.first(rec, "ring", 1), m.ring_state(), name)
    check_stamps(ref_ring.first(rec, "stamps", 1), m.stamps(), name)
    got = m.dump_state()
    ref_state = ref_ring.first(rec, "state")
    stage = STAGE_NO[sc["stop_after"]]
    if sc["fusion"] == "neighbours":
        thr = PARAMS["occupancy_threshold"]
        rows = [m.fusion_neighbors(v, thr) for v in sc["fusion_voxels"]]
        fus = ref_ring.first(rec, "fusion")
        for k, key in enumerate(("wsum", "guessed")):
            g = np.array([r[k] for r in rows], np.float32)
            assert np.array_equal(bits(fus[key]), bits(g)), (key, np.flatnonzero(bits(fus[key]) != bits(g))[:8])
        assert [r[2] for r in rows] == fus["label"].tolist() and [r[3] for r in rows] == fus["track"].tolist()
        inferred = np.float32(np.float32(thr) + np.float32(0.1))
        assert (fus["wsum"] == inferred).any() and (fus["wsum"] == 0).any() and (fus["wsum"] == -1).any(), "a branch of the fusion is not hit"
        got = m.dump_state()
    if name == "move_overflow":
        # recorded deviation (move_overflow_scenario): which of the object's particles won the slots of the target voxel is
        # the walk order of its set.  Everything else is compared: every other voxel in full, and in the target voxel
        # the multiset of the survivors' fields other than position, which the scenario makes independent of that order.
        ref, before = dense(cfg, ref_state), sc["state"]
        target = int(sc["target_voxel"])
        assert np.array_equal(ref["status"], got["status"]), np.flatnonzero(ref["status"] != got["status"])[:8]
        check_state(sc, ref_state, got, name, skip_voxels=[target])
        own = before["owner"] == 21
        assert (ref["status"][target * s + 1:(target + 1) * s] != INVALID).all() and own.sum() > s - 1, "the voxel does not overflow"
        ref_rows, got_rows = survivors(cfg, ref, target), survivors(cfg, got, target)
        assert ref_rows == got_rows, (ref_rows, got_rows)
        assert len(set(ref_rows)) == 2 and len(ref_rows) == s - 1, "the bystander and the object's particles are not both there"
        # positions: the bystander's is untouched; each survivor of the object is one of its particles, moved, and none twice
        t = np.asarray(sc["moves"][0][1], F)[:3, 3]
        moved = set((before["px"][i] + t[0], before["py"][i] + t[1], before["pz"][i] + t[2]) for i in np.flatnonzero(own))
        assert len(moved) == own.sum()
        j = int(np.flatnonzero(~own & (before["idx"] // s == target) & (before["idx"] % s != 0))[0])
        for st in (ref, got):
            at = [i for i in range(target * s + 1, (target + 1) * s)]
            pos = [(st["px"][i], st["py"][i], st["pz"][i]) for i in at]
            mine = [p for i, p in zip(at, pos) if st["track"][i] == 21]
            rest = [p for i, p in zip(at, pos) if st["track"][i] != 21]
            assert len(set(mine)) == len(mine) == s - 2 and set(mine) <= moved, (mine, sorted(moved))
            assert rest == [(before["px"][j], before["py"][j], before["pz"][j])], rest
        return
    skip = list(sc.get("ambiguous_idx", ()))
    skip_voxels = sorted(set(int(i) // s for i in skip))     # an ambiguous particle can decide whether its voxel was observed
    check_state(sc, ref_state, got, name, skip_idx=skip, skip_voxels=skip_voxels, pos_tol=None if sc["exact"] else FLOAT_TOL["pos"])
    if stage >= 4:
        ref_bins = ref_ring.first(rec, "bins")
        assert ref_ring.first(rec, "visible") == 1
        got_bins = split_bins(m)
        if not bins_ordered:
            ref_bins = {p: np.sort(b) for p, b in ref_bins.items()}
        check_bins(ref_bins, got_bins, name, ordered=True, skip_idx=skip)
        if name.startswith("visible"):
            assert sum(len(b) for b in ref_bins.values()) > 20, "the view bins next to nothing"
    if sc["fusion"] == "plain":
        check_wsum(sc, ref_ring.first(rec, "fusion"), m.voxels()["wsum"][sc["fusion_voxels"]], name)
    elif stage >= 7:
        occ = ref_ring.first(rec, "occupancy")
        check_occupancy(sc, occ, m.voxels(), name)
        assert set(occ["rows"][:, 1]) == {0, 1, 2}, "free, occupied and guessed-occupied voxels are not all there"
