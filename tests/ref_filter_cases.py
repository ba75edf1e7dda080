"""Scenarios that hold the oracle and the HIP library to the reference's own filter: updateParticles, the birth members
and resampleParticlesInVoxel of semantic_dsp_map.h over ObjectParticleHashMap, compiled over oracle/ref_shims/ and driven
by oracle/ref_filter_harness.cpp.  Built with plain numpy, regenerated from seeds, and small.

A scenario is a dict; `scripts(sc)` gives the commands of its harness runs, `make_map` / `run_frame` / `run_two_frames`
run it through the common Python surface of oracle.OracleMap and binding.SdmMap, and the `check_*` functions compare
either with what the reference answered (tests/golden/ref_filter_<variant>.npz, tests/golden/make_golden_ref_filter.py).

The camera looks down +z from `pos` with the identity orientation; a particle or a point "at pixel (r, c), depth z" sits
at the centre of that pixel (cam_point), far from any border a float could decide differently.  The depth image is one
constant beyond every particle, so the visibility pass bins them all; the cloud is given to the filter as it is.

exact scenarios: no sum has a second term whose order could matter (weight_single), or every sum is of dyadic weights
(resample_direct, birth_*, cursor_wrap, two_frames, guessed) - everything is compared bit for bit.
The others (weight_window_edges, weight_forget, weight_random_*): integers exactly, weights within weight_tol().
"""
import numpy as np

from oracle import ref_filter
from tests import ref_ring_cases as rc
from tests.ref_ring_cases import COPIED, F, GUESSED_BORN, IDENT_Q, INVALID, NO_TRACK, REGULAR_BORN, UPDATED, dims, lat  # noqa: F401

MAX_MOVABLE = 65523
STATIC_A, STATIC_B = 65530, 65529          # Building, Road: instance ids above g_max_movable_object_instance_id
DEPTH = 6.0
NOISE_PERIOD = 1024
GAUSSIAN_RANDOM_NUM = 1000000

# Largest difference of a float output between an -O0 and an -O3 -march=native -ffp-contract=off build of the harness
# (`make -C oracle ref-spread`, tests/golden/make_golden_ref_filter.py --spread): 0.0 with identical answers in every
# scenario of every variant but one - t0 weight_random_0, where one weight of 901 comes out two ulps (2.98e-8) lower in the
# -O0 build.  The -O3 -march=native build, the build of the fixtures and the oracle agree on it bit for bit, so the oracle,
# which sums in the reference's order, is held bit for bit and this number is used by no comparison.
MEASURED_SPREAD = 2.98023e-08

# Largest relative difference of a particle weight among the reference's own three permute_bins runs (as pushed,
# ascending, reversed) of a scenario, per variant (make_golden_ref_filter.py prints them; test_oracle_filter_vs_reference
# recomputes them from the fixtures and asserts these are the values).  The library sums in a fourth order (row partial
# sums), hence the factor 4; never looser than the 1e-4 of tests/test_parity_gpu.py, never tighter than one ulp.
MEASURED_ORDER_SPREAD = {
    "zed2_boost": {"weight_forget_independent": 0.0, "weight_window_edges": 2.1987793256695613e-07, "weight_forget": 0.0, "weight_random_0": 7.754925734953699e-07, "weight_random_1": 3.241559909942983e-07},
    "t1": {"weight_forget_independent": 0.0, "weight_window_edges": 0.0, "weight_forget": 0.0, "weight_random_0": 4.916374920784909e-07, "weight_random_1": 1.645229328516102e-07},
    "t0": {"weight_forget_independent": 0.0, "weight_window_edges": 0.0, "weight_forget": 0.0, "weight_random_0": 4.396134508234473e-07, "weight_random_1": 1.9256037842992557e-07},
}
ORDER_FACTOR = 4.0
ORDER_CAP = 1e-4
ULP = 2.0 ** -23                            # relative spacing of binary32
AMBIGUOUS_CAP = 0.01


def weight_tol(variant, name):
    """relative tolerance of a weight of a non-exact scenario; check_particles adds the floor, one ulp of the largest weight"""
    tol = ORDER_FACTOR * MEASURED_ORDER_SPREAD[variant][name]
    assert tol <= ORDER_CAP, "%s %s: 4 x the reference's own order spread exceeds 1e-4 - change the scenario, not the bound" % (variant, name)
    return tol


def params(**kw):
    p = dict(rc.PARAMS)
    p.update(kw)
    return p


def window_half(variant):
    """semantic_dsp_map.h:964-970: 3 under BOOST_MODE 1, 5 otherwise.  All three ring variants are the SETTING 3 block with
    its BOOST_MODE 1 (that is what halves their images), so the reference's window is 7 x 7 in every one of them."""
    return 3


def config(variant):
    """the project's configuration of a variant with the window the reference uses there (T1 itself asks for 11 x 11) and
    the g_max_movable_object_instance_id the reference starts with (data_base.h:196), which holds until an object csv is
    read (object_info_handler.h:84; the shipped one lowers it by one) - the harness reads none"""
    return dict(rc.config(variant), window_half=window_half(variant), max_movable_track=MAX_MOVABLE)


# ------------------------------------------------------------------------------------------------ building
def cam_point(cfg, pos, r, c, z, du=0.5, dv=0.5):
    return np.array([float(pos[0]) + (c + du - cfg["cx"]) * z / cfg["fx"], float(pos[1]) + (r + dv - cfg["cy"]) * z / cfg["fy"], float(pos[2]) + z], F)


class Builder:
    def __init__(self, variant):
        self.variant = variant
        self.cfg = config(variant)
        self.n, self.s = dims(self.cfg)
        self.pos = np.array([lat(self.cfg, 4), lat(self.cfg, 4), lat(self.cfg, 4)], F)     # half a voxel off the lattice
        self.ts = 3
        self.st = rc.Sparse(self.cfg)
        self.cloud = {}

    def particle_at(self, p, w, track=NO_TRACK, label=1, forget=0, status=UPDATED, slot=None):
        v = rc.voxel_of(self.cfg, self.pos, p)
        assert v is not None, "a particle outside the map"
        idx = self.st.free_slot(v) if slot is None else v * self.s + slot
        assert idx is not None, "voxel %d is full" % v
        owner = track if track <= MAX_MOVABLE else NO_TRACK
        return self.st.put(idx, p, w=w, ts=self.ts - 1, track=track, label=label, status=status, forget=forget, owner=owner)

    def particle(self, r, c, z, w, du=0.5, dv=0.5, **kw):
        return self.particle_at(cam_point(self.cfg, self.pos, r, c, z, du, dv), w, **kw)

    def point(self, r, c, z=None, sigma=0.2, label=1, track=NO_TRACK, valid=True, p=None):
        assert (r, c) not in self.cloud and 0 <= r < self.cfg["height"] and 0 <= c < self.cfg["width"], (r, c)
        if p is None:
            p = cam_point(self.cfg, self.pos, r, c, z)
        self.cloud[(r, c)] = (r, c, F(p[0]), F(p[1]), F(p[2]), F(sigma), int(label), int(track), bool(valid))

    def cell_centre(self, cell, frac=(0.5, 0.5, 0.5)):
        return rc.cell_pos(self.cfg, self.pos, cell, frac)

    def frame(self, name, exact, prm, births=False, orders=(0,), noise=(0.0,), burn=0, default_sigma=0.2, **extra):
        cfg = self.cfg
        sc = dict(name=name, variant=self.variant, kind="frame", exact=exact, params=prm, path=[self.pos], pos=self.pos, q=IDENT_Q, ts=self.ts,
                  state=self.st.arrays(), depth=np.full((cfg["height"], cfg["width"]), DEPTH, F), cloud=[self.cloud[k] for k in sorted(self.cloud)],
                  default_sigma=F(default_sigma), noise=np.asarray(noise, F), burn=burn, orders=tuple(orders), births=births)
        sc["extrinsic"] = rc.extrinsic(self.pos, IDENT_Q)
        sc.update(extra)
        return sc


def index_noise():
    """a table whose entries say where they are: entry i = ((37 i mod 1024) - 512) * 2^-14, a bijection of i mod 1024; with
    a sigma of 2^-2 a newborn's offset from its point is one of 1024 multiples of 2^-16, below a centimetre"""
    i = np.arange(NOISE_PERIOD)
    return (((37 * i) % NOISE_PERIOD - NOISE_PERIOD // 2) * 2.0 ** -14).astype(F)


# ------------------------------------------------------------------------------------------------ weight scenarios
def weight_single(variant, independent):
    """lines 1009-1029, 1076-1113 with one term per sum: pairs of one particle and one valid point, so far from every
    other pair that no window holds a second particle and no particle sees a second point.  Same and different track,
    forget counts 0, 1 and 5, in either state of if_use_independent_filter."""
    b = Builder(variant)
    cfg, h = b.cfg, window_half(variant)
    step = 2 * (2 * h + 1) + 2
    combos = [(same, forget) for same in (True, False) for forget in (0, 1, 5)]
    k = 0
    rows = range(h + 1, min(cfg["height"], 4 * step) - h - 1, step)
    cols = range(h + 1, min(cfg["width"], 6 * step) - h - 1, step)
    r_off, c_off = (cfg["height"] - (rows[-1] + h + 2)) // 2, (cfg["width"] - (cols[-1] + h + 2)) // 2     # centred: visible at any size
    for r in rows:
        for c in cols:
            same, forget = combos[k % len(combos)]
            dr, dc = [(0, 0), (h, -h), (-h, h), (2, -1), (-3, h), (h, 0)][k % 6]
            z = 2.5 + 0.25 * (k % 5)
            track = [3, STATIC_A, 4][k % 3]
            b.particle(r + r_off, c + c_off, z + 0.0625 * (k % 3), (1 + k % 40) / 64.0, track=track, label=2 + k % 9, forget=forget)
            b.point(r + r_off + dr, c + c_off + dc, z, sigma=0.25, label=5, track=track if same else [4, 3, STATIC_B][k % 3])
            k += 1
    assert k >= 12, "too few pairs: %d" % k
    return b.frame("weight_single_%d" % independent, True, params(if_use_independent_filter=independent))


def weight_window_edges(variant):
    """the window bounds of lines 989-998 and 1061-1074: particles and points in the first and last rows and columns, at
    distance exactly window_half (inside) and window_half + 1 (outside); invalid pixels inside windows; and a pixel that
    holds particles but is itself invalid, whose stated sigma differs from its neighbours' (line 1047 reads it)."""
    b = Builder(variant)
    cfg, h = b.cfg, window_half(variant)
    H, W = cfg["height"], cfg["width"]
    z = 3.0
    # zed2_boost's image is wider than its map at 3 m: its corners are the corners of the part that the BFS reaches
    r0, r1, c0, c1 = (0, H - 1, 0, W - 1)
    if variant == "zed2_boost":
        c0, c1 = W // 2 - 150, W // 2 + 150
    k = 0
    for (r, c, sr, sc_) in ((r0, c0, 1, 1), (r0, c1, 1, -1), (r1, c0, -1, 1), (r1, c1, -1, -1)):
        for j in range(3):
            b.particle(r, c, z + 0.0625 * j, (10 + 7 * j + k) / 64.0, track=[3, STATIC_A, 3][j], label=3 + j, forget=j, du=0.25 + 0.25 * j)
        b.point(r, c, z, sigma=0.25, label=5, track=3)
        b.point(r + sr * h, c, z + 0.05, sigma=0.25, label=5, track=3)                   # exactly window_half down / up
        b.point(r, c + sc_ * h, z - 0.05, sigma=0.3, label=6, track=STATIC_A)            # exactly window_half sideways
        b.point(r + sr * (h + 1), c, z, sigma=0.25, label=5, track=3)                    # one further: outside the window
        b.point(r, c + sc_ * (h + 1), z, sigma=0.25, label=5, track=3)
        b.point(r + sr * h, c + sc_ * h, z + 0.1, sigma=0.2, label=7, track=4)           # the window's corner
        b.point(r + sr * 2, c + sc_ * 2, z, sigma=0.9, label=0, track=0, valid=False)    # invalid inside the window
        b.particle(r + sr * (h + 1), c + sc_ * 1, z + 0.02, 0.375, track=3, label=4)     # seen from (r, c)'s far neighbours only
        k += 1
    # the middle: an invalid pixel that holds particles, sigma 0.35 against the 0.2 of the points round it
    rm, cm = H // 2, (c0 + c1) // 2
    b.point(rm, cm, z, sigma=0.35, label=0, track=0, valid=False)
    for j in range(3):
        b.particle(rm, cm, z + 0.05 * j, (20 + j) / 64.0, track=[3, 4, STATIC_A][j], label=2, forget=j % 2, du=0.25 + 0.25 * j)
    for dr, dc in ((0, 1), (1, 0), (-1, -1), (h, h), (-h, 0), (0, -h), (h + 1, 0), (2, -3)):
        b.point(rm + dr, cm + dc, z + 0.01 * dr, sigma=0.2, label=5, track=[3, 4, STATIC_A][(dr + dc) % 3])
    b.particle(rm + 1, cm + 1, z + 0.35, 0.25, track=4, label=2)
    b.particle(rm - h, cm, z - 0.4, 0.5, track=3, label=2, forget=1)
    return b.frame("weight_window_edges", False, params(if_use_independent_filter=0, max_forget_count=5), orders=(0, 1, 2), default_sigma=0.2,
                   edge_pixels=[(r0, c0), (r0, c1), (r1, c0), (r1, c1)], invalid_holder=(rm, cm))


def weight_forget(variant):
    """lines 1089-1096 and 1107-1113: gk well above and well below c_min_rightly_updated_pdf (0.1) for matching and other
    tracks, forget counts 0 to 5, max_forget_count = 3 - getForgettingFactor uses the parameter (counts 3, 4, 5 weigh
    nothing), the cap of line 1111 is the literal 5 (4 becomes 5, 5 stays).  A max_forget_count above 5 would make the
    reference read forgetting_function[5], out of bounds, for a count of 5; that is not asked of it."""
    b = Builder(variant)
    cfg, h = b.cfg, window_half(variant)
    step = max(2 * h + 4, 16)                        # pairs in voxels of their own, whatever the variant's voxel size
    r0, c0 = cfg["height"] // 2 - 2 * step, cfg["width"] // 2 - 3 * step
    k = 0
    for i in range(4):
        for j in range(6):
            r, c = r0 + i * step + h, c0 + j * step + h
            forget = [0, 1, 2, 3, 4, 5][j]
            same = i % 2 == 0
            near = i < 2
            z = 3.0
            sigma = 0.25
            # near: the point's own pixel and depth, gk = pdf(small)^3 about 0.17; far: two sigma off in depth, about 0.02
            b.particle(r, c, z if near else z + 2.0 * sigma, (8 + 3 * k % 40) / 64.0, track=3, label=14, forget=forget)
            b.particle(r, c, z + 0.03 if near else z + 2.1 * sigma, 0.25, track=STATIC_A, label=6, forget=forget, du=0.25)
            b.point(r, c, z, sigma=sigma, label=14 if same else 15, track=3 if same else 4)
            b.point(r + 1, c - 2, z + 0.01, sigma=sigma, label=6, track=STATIC_A if same else STATIC_B)
            k += 1
    return b.frame("weight_forget", False, params(if_use_independent_filter=0, max_forget_count=3, forgetting_rate=2.0), orders=(0, 1, 2))


def weight_forget_independent(variant):
    """line 1107: in independent mode forget_count is left alone, whatever gk is"""
    sc = weight_forget(variant)
    sc["name"] = "weight_forget_independent"
    sc["params"] = params(if_use_independent_filter=1, max_forget_count=3, forgetting_rate=2.0)
    return sc


WEIGHT_RANDOM_SEED = {"zed2_boost": 5, "t1": 5, "t0": 5}


def weight_random(variant, independent):
    """a seeded surface of a few thousand valid points with a few invalid ones, and particles scattered about it in
    depth, several to a pixel, of three tracks and all forget counts"""
    b = Builder(variant)
    cfg = b.cfg
    rng = np.random.default_rng(WEIGHT_RANDOM_SEED[variant] + independent)
    H, W = cfg["height"], cfg["width"]
    bh, bw = min(H - 4, 44), min(W - 4, 64)
    r0, c0 = (H - bh) // 2, (W - bw) // 2
    tracks = [3, 4, STATIC_A]
    for r in range(r0, r0 + bh):
        for c in range(c0, c0 + bw):
            z = 2.6 + 0.9 * (c - c0) / bw + 0.3 * np.sin(0.4 * r) + rng.normal(0, 0.01)
            valid = rng.random() > 0.06
            tr = tracks[0] if c < c0 + bw // 3 else tracks[1] if c < c0 + 2 * bw // 3 else tracks[2]
            b.point(r, c, z, sigma=float(F(0.15 + 0.1 * rng.random())), label=14 if tr <= MAX_MOVABLE else 6, track=tr, valid=valid)
    want, made, tries = 900, 0, 0
    while made < want and tries < 40 * want:
        tries += 1
        r, c = int(rng.integers(r0 - 3, r0 + bh + 3)), int(rng.integers(c0 - 3, c0 + bw + 3))
        zs = 2.6 + 0.9 * (min(max(c, c0), c0 + bw - 1) - c0) / bw + 0.3 * np.sin(0.4 * r)
        for j in range(int(rng.integers(1, 4))):                         # several to a pixel, at different depths
            p = cam_point(cfg, b.pos, r, c, zs + rng.normal(0, 0.25), 0.2 + 0.6 * rng.random(), 0.2 + 0.6 * rng.random())
            v = rc.voxel_of(cfg, b.pos, p)
            if v is None or b.st.free_slot(v) is None:
                continue
            b.particle_at(p, float(F(rng.uniform(0.05, 1.0))), track=int(rng.choice(tracks)), label=int(rng.integers(1, 16)), forget=int(rng.integers(0, 6)),
                          status=int(rng.choice([UPDATED, UPDATED, REGULAR_BORN, COPIED])))
            made += 1
    return b.frame("weight_random_%d" % independent, False, params(if_use_independent_filter=independent, max_forget_count=5), orders=(0, 1, 2))


# ------------------------------------------------------------------------------------------------ births
BIRTH_KINDS = ("fills", "full", "to_empty", "heavy", "empty", "over_half", "full_static")
PHASES = [(2, 2), (0, 1), (1, 0), (0, 0), (2, 1), (1, 2), (0, 2), (1, 1), (2, 0)]      # not the order the loop visits them in


def birth(variant, name, depth_noise, nb, burn=0):
    """visible, update_particles, births.  Independent filter on, the stored particles of tracks (7, STATIC_B) that no
    point carries, detection_probability 0.5: every visible weight is multiplied by exactly 0 * 0.5 + 1 - 0.5 (lines
    1009-1014, 1103), and with dyadic weights every sum of the resampling is exact.

    One voxel per kind and point track, the points of a voxel in pixels of different phases of the 3 x 3 interleaved
    loop, listed in an order that is not the loop's:
      fills        S/2 stored (no resampling: not MORE than S/2), more points than vacant slots: the voxel fills up mid-loop
      full         every slot stored: the first insertion fails; plain: resampled after it all the same; noise: resampled
                   because of it, and the insertion tried again
      to_empty     every slot stored, weight sum below 0.01: resampled to empty, then born into
      heavy        one particle far heavier than the rest: weight_per_particle clipped at 1, several thresholds passed
      empty        nothing stored, more points than slots: newborns are not UPDATED, so nothing is ever resampled
      over_half    S/2 + 1 stored: plain resamples after the first insertion, noise only once the voxel is full
      full_static  as full with stored particles of a static track: no owner set to take them from
    """
    b = Builder(variant)
    cfg, s = b.cfg, b.s
    U, Hf = s - 1, s >> 1
    mid = [k >> 1 for k in b.n]
    dz0 = int(round(3.0 / float(F(cfg["voxel_size"]))))
    cells = [(mid[0] + dx, mid[1] + dy, mid[2] + dz0 + dz) for dz in (0, 2) for dy in (-1, 1) for dx in (-3, -1, 1, 3)]
    point_tracks = [3, STATIC_A, 4]
    sigma = 0.25
    vox = []
    for i, cell in enumerate(cells[:14] if len(cells) >= 14 else cells):
        kind = BIRTH_KINDS[i % len(BIRTH_KINDS)]
        stored_track = STATIC_B if kind == "full_static" else 7
        n_stored = {"fills": Hf, "full": U, "to_empty": U, "heavy": U, "empty": 0, "over_half": Hf + 1, "full_static": U}[kind]
        n_points = {"fills": U - Hf + 2, "full": 3, "to_empty": 3, "heavy": 3, "empty": U + 2, "over_half": 3, "full_static": 3}[kind]
        if depth_noise and nb > 1:
            n_points = max(2, (n_points + 1) // 2)                     # three newborns to a point
        for j in range(n_stored):
            w = {"to_empty": 1 / 512.0, "heavy": 6.0 if j == 1 else 4 / 64.0}.get(kind, (6 + 5 * ((i + j) % 4)) / 64.0)
            b.particle_at(b.cell_centre(cell, (0.25 + 0.0625 * j, 0.5, 0.75 - 0.0625 * j)), w, track=stored_track, label=2 + j % 3, forget=j % 3)
        v = rc.voxel_of(cfg, b.pos, b.cell_centre(cell))
        vox.append((v, kind))
        for j in range(n_points):
            pr, pc = PHASES[j % 9]
            r, c = 9 + 12 * (i // 8) + 3 * (j // 9) + pr, 4 + 6 * (i % 8) + pc
            tr = point_tracks[(i + j // 2) % 3]
            b.point(r, c, sigma=sigma, label=14 if tr <= MAX_MOVABLE else 6, track=tr, p=b.cell_centre(cell, (0.5, 0.375 + 0.03125 * j, 0.5)))
    prm = params(detection_probability=0.5, if_use_independent_filter=1, if_consider_depth_noise=depth_noise, nb_ptc_num_per_point=nb)
    return b.frame(name, True, prm, births=True, noise=index_noise() if depth_noise else (0.0,), burn=burn, voxels=vox)


def two_frames(variant):
    """two consecutive frames that carry the noise cursor and the owner sets: the first is birth_noise's; before the
    second, object 3 - the particles born for it in the first - is moved one voxel down the optical axis
    (semantic_dsp_map.h:587-699: moveParticlesInSetsByTransformations on the object's owner set, then
    updatePtcIndicesOfObj), and points of other tracks are born into voxels it never touches.  A wrong owner set shows
    up as particles that did not move.  One repeated noise value: the move draws noise too, per particle in the walk
    order of the set, which is std::unordered_set order in the reference (check_two_frames has the branch)."""
    sc = birth(variant, "two_frames", 1, 3)
    b = Builder(variant)
    cfg = b.cfg
    mid = [k >> 1 for k in b.n]
    dz0 = int(round(3.0 / float(F(cfg["voxel_size"]))))
    move = np.eye(4, dtype=F)
    move[2, 3] = lat(cfg, 8)                                           # one voxel along z: into cells no scenario voxel uses
    for j, (dx, tr) in enumerate([(0, STATIC_A), (0, 4), (2, STATIC_B), (-2, 9)]):
        cell = (mid[0] + dx, mid[1] + (j % 2), mid[2] + dz0 + 1)
        b.point(20 + j % 3, 30 + 4 * j + (j + 1) % 3, sigma=0.25, label=14 if tr <= MAX_MOVABLE else 6, track=tr, p=b.cell_centre(cell, (0.5, 0.5, 0.375)))
    sc.update(kind="two_frames", noise=np.array([2.0 ** -6], F), moved_track=3, move=move, cloud2=[b.cloud[k] for k in sorted(b.cloud)])
    return sc


# ------------------------------------------------------------------------------------------------ direct calls
def resample_direct(variant):
    """resampleParticlesInVoxel (lines 1448-1519) on crafted voxels; dyadic weights, every sum exact"""
    b = Builder(variant)
    cfg, s = b.cfg, b.s
    U, Hf = s - 1, s >> 1
    mid = [k >> 1 for k in b.n]
    cases = []

    def voxel(i, weights, statuses=None, tracks=None):
        cell = (mid[0] - 4 + i % 8, mid[1] + (i // 8), mid[2] + 2)
        for j, w in enumerate(weights):
            st = UPDATED if statuses is None else statuses[j]
            if st == INVALID:
                continue
            tr = 7 if tracks is None else tracks[j]
            b.particle_at(b.cell_centre(cell, (0.25, 0.25 + 0.0625 * j, 0.5)), w, track=tr, label=3, status=st, slot=1 + j)
        cases.append(rc.voxel_of(cfg, b.pos, b.cell_centre(cell)))

    voxel(0, [0.25] * Hf)                                                   # exactly S/2 UPDATED: not more than S/2, untouched
    voxel(1, [0.25] * (Hf + 1))                                             # S/2 + 1
    voxel(2, [(2 if j < 5 - (Hf + 1) else 1) / 512.0 for j in range(Hf + 1)])     # sum 5/512 = 0.00977 < 0.01: emptied
    voxel(3, [(2 if j < 6 - (Hf + 1) else 1) / 512.0 for j in range(Hf + 1)])     # sum 6/512 = 0.01172: resampled
    voxel(4, [1.5] * U)                                                     # weight_per_particle clipped at 1
    voxel(5, [1 / 64.0, 40 / 64.0] + [1 / 64.0] * (U - 2))                  # one heavy particle passes several thresholds
    voxel(6, [0.125 * (1 + j % 3) for j in range(U)], tracks=[[7, 9, STATIC_A][j % 3] for j in range(U)])     # two owners and a static track
    voxel(7, [3 / 64.0, 0.5, 5 / 64.0] + [0.25] * (U - 3))
    if U >= Hf + 3:                                                         # room for slots that are not UPDATED in between (8 slots only)
        st = [UPDATED, COPIED, UPDATED, INVALID] + [UPDATED] * (U - 4)
        voxel(8, [0.25, 0.5, 0.125, 0.0] + [0.1875] * (U - 4), statuses=st)
        st = [REGULAR_BORN, UPDATED, GUESSED_BORN] + [UPDATED] * (U - 3)
        voxel(9, [0.05, 0.375, 0.05] + [0.25] * (U - 3), statuses=st, tracks=[9] * U)
    return dict(name="resample_direct", variant=variant, kind="resample", exact=True, params=params(), path=[b.pos], pos=b.pos, ts=b.ts,
                state=b.st.arrays(), voxels=cases, noise=np.zeros(1, F))


def guessed(variant):
    """addGuessedParticle (lines 1126-1142): a movable track (owner set), a static one (none), into a full voxel, outside"""
    b = Builder(variant)
    cfg, s = b.cfg, b.s
    mid = [k >> 1 for k in b.n]
    full = (mid[0] + 2, mid[1], mid[2] + 3)
    for j in range(s - 1):
        b.particle_at(b.cell_centre(full, (0.25, 0.5, 0.5)), 0.25, track=7, label=3)
    groups = []
    pts = [b.cell_centre((mid[0] - 1, mid[1], mid[2] + 3), (0.125 * (k + 1), 0.5, 0.25)) for k in range(3)] + [b.cell_centre(full)]
    groups.append((14, 5, np.array(pts, F)))
    pts = [b.cell_centre((mid[0] - 1, mid[1], mid[2] + 3), (0.5, 0.125 * (k + 1), 0.75)) for k in range(2)]
    pts += [b.cell_centre((3 * b.n[0], mid[1], mid[2]))]
    groups.append((6, STATIC_A, np.array(pts, F)))
    groups.append((15, MAX_MOVABLE, np.array([b.cell_centre((mid[0], mid[1] + 1, mid[2] + 4))], F)))          # the last movable id
    groups.append((12, MAX_MOVABLE + 1, np.array([b.cell_centre((mid[0], mid[1] + 1, mid[2] + 4), (0.25, 0.25, 0.25))], F)))
    return dict(name="guessed", variant=variant, kind="guessed", exact=True, params=params(), path=[b.pos], pos=b.pos, ts=b.ts,
                state=b.st.arrays(), groups=groups, noise=np.zeros(1, F))


# ------------------------------------------------------------------------------------------------ the list
def scenarios(variant):
    return [weight_single(variant, 0), weight_single(variant, 1), weight_window_edges(variant), weight_forget(variant),
            weight_forget_independent(variant), weight_random(variant, 0), weight_random(variant, 1), resample_direct(variant),
            birth(variant, "birth_plain", 0, 3), birth(variant, "birth_noise", 1, 3), birth(variant, "birth_noise_nb1", 1, 1),
            birth(variant, "cursor_wrap", 1, 3, burn=GAUSSIAN_RANDOM_NUM - 5), two_frames(variant), guessed(variant)]


NAMES = ["weight_single_0", "weight_single_1", "weight_window_edges", "weight_forget", "weight_forget_independent", "weight_random_0",
         "weight_random_1", "resample_direct", "birth_plain", "birth_noise", "birth_noise_nb1", "cursor_wrap", "two_frames", "guessed"]
GPU_FRAMES = [n for n in NAMES if n not in ("resample_direct", "guessed", "two_frames")]      # direct calls: the library has no entry for them


# ------------------------------------------------------------------------------------------------ harness scripts
def owners_of(sp):
    own = {}
    for i, t in zip(sp["idx"], sp["owner"]):
        if t != NO_TRACK:
            own.setdefault(int(t), []).append(int(i))
    return own


def _head(sc):
    s = ref_filter.Script()
    s.noise(sc["noise"])
    s.params(sc["params"])
    s.ts(1)
    s.ego(sc["path"][0])
    s.dump("ring", "stamps")
    return s


def _frame_commands(s, sc, cloud, order=0, bins=True):
    s.visible(sc["extrinsic"], sc["depth"])
    if bins:
        s.dump("bins")
    s.cloud(sc["default_sigma"], cloud)
    s.permute_bins(order)
    s.update_particles()
    s.dump("particles")


def two_frames_scripts(sc, answers):
    """the harness has one map per process and the reference keeps the moved set in a local, so the second frame takes
    three runs: "" is the first frame and says which particles object 3 owns; "b" repeats it and moves them, which says
    where they went; "c" repeats both, hands that set to updatePtcIndicesOfObj and runs the second frame"""
    def first_frame():
        s = _head(sc)
        s.load(sc["state"])
        s.set_owners(owners_of(sc["state"]))
        s.ts(sc["ts"])
        s.ego(sc["pos"])
        _frame_commands(s, sc, sc["cloud"])
        s.births(-1)
        s.dump("particles", "cursor", "owners")
        return s
    out = {"": first_frame().text()}
    if "" in answers:
        owned = ref_filter.first(ref_filter.parse(answers[""]), "owners")[sc["moved_track"]]
        s = first_frame()
        s.ts(sc["ts"] + 1)
        s.ego(sc["pos"])
        s.move([owned], [sc["move"]])
        out["b"] = s.text()
        if "b" in answers:
            moved = ref_filter.first(ref_filter.parse(answers["b"]), "move")[0]
            s.set_owners({sc["moved_track"]: moved})
            _frame_commands(s, sc, sc["cloud2"], bins=False)
            s.births(-1)
            s.dump("particles", "cursor", "owners")
            out["c"] = s.text()
    return out


def scripts(sc, answers=None):
    """{key: commands}: "" is the run the comparison uses; "o1", "o2" the same weight stage with every per-pixel list
    sorted / reversed, the reference's own word on how much its answer hangs on the order of its sums.  answers: what
    the harness said to the runs before, {key: text}, for the one scenario whose later runs need it (two_frames)."""
    out = {}
    if sc["kind"] == "two_frames":
        return two_frames_scripts(sc, answers or {})
    if sc["kind"] == "resample":
        s = _head(sc)
        s.load(sc["state"])
        s.set_owners(owners_of(sc["state"]))
        s.ts(sc["ts"])
        s.resample(sc["voxels"])
        s.dump("particles", "owners")
        return {"": s.text()}
    if sc["kind"] == "guessed":
        s = _head(sc)
        s.load(sc["state"])
        s.set_owners(owners_of(sc["state"]))
        s.ts(sc["ts"])
        for label, track, pts in sc["groups"]:
            s.guessed(pts, label, track)
        s.dump("particles", "owners")
        return {"": s.text()}
    for order in sc["orders"]:
        s = _head(sc)
        if sc["burn"]:
            s.burn(sc["burn"])
        s.load(sc["state"])
        s.set_owners(owners_of(sc["state"]))
        s.ts(sc["ts"])
        s.ego(sc["pos"])
        _frame_commands(s, sc, sc["cloud"], order, bins=order == 0)
        if sc["births"] and order == 0:
            s.births(-1)
            s.dump("particles", "cursor", "owners")
        out["" if order == 0 else "o%d" % order] = s.text()
    return out


# ------------------------------------------------------------------------------------------------ running a map
def cloud_array(sc, key="cloud"):
    cfg = config(sc["variant"])
    cloud = np.zeros(cfg["width"] * cfg["height"], rc.LP)
    cloud["sigma"] = sc["default_sigma"]
    for r, c, x, y, z, sigma, label, track, valid in sc[key]:
        pt = cloud[r * cfg["width"] + c:r * cfg["width"] + c + 1]
        pt["x"], pt["y"], pt["z"], pt["sigma"], pt["label_id"], pt["track_id"], pt["is_valid"] = x, y, z, sigma, label, track, valid
    return cloud


def make_map(make, sc, rec, gts, bin_order=0):
    cfg = config(sc["variant"])
    m = make(dict(cfg, bin_order=bin_order), sc["params"], rc.noise_table(sc))
    m.load_state(rc.dense(cfg, sc["state"]))
    ring = rc.ring_dict(ref_filter.first(rec, "ring", 0), gts)
    ring["birth_cursor"] = sc.get("burn", 0)
    m.set_ring_state(ring)
    m.set_stamps(*ref_filter.first(rec, "stamps", 0))
    return m


def run_frame(make, sc, rec, stop_after, bin_order=0):
    m = make_map(make, sc, rec, sc["ts"] - 1, bin_order)
    m.update(sc["depth"].reshape(-1), cloud_array(sc), sc["pos"], sc["q"], stop_after=stop_after)
    return m


def run_two_frames(make, sc, rec):
    """both frames on one map, each stopped after its births (the harness has no occupancy sweep between them either)"""
    m = make_map(make, sc, rec, sc["ts"] - 1)
    m.update(sc["depth"].reshape(-1), cloud_array(sc), sc["pos"], sc["q"], stop_after="birth")
    moves = np.zeros(1, rc.OBJECT_MOVE)
    moves[0]["track_id"], moves[0]["T"] = sc["moved_track"], np.asarray(sc["move"], F).reshape(-1)
    m.update(sc["depth"].reshape(-1), cloud_array(sc, "cloud2"), sc["pos"], sc["q"], moves, stop_after="birth")
    return m


# ------------------------------------------------------------------------------------------------ comparisons
bits = rc.bits


def order_spread(recs):
    """largest relative difference of a weight among the state dumps after update_particles of the reference's runs
    (as pushed, sorted, reversed), and the slots whose integers differ among them"""
    states = [ref_filter.first(r, "particles", 0) for r in recs]
    a = states[0]
    worst, differ = 0.0, set()
    for o in states[1:]:
        assert np.array_equal(a["idx"], o["idx"])
        w0, w1 = a["w"].astype(np.float64), o["w"].astype(np.float64)
        nz = np.maximum(np.abs(w0), np.abs(w1)) > 0
        if nz.any():
            worst = max(worst, float((np.abs(w0 - w1)[nz] / np.maximum(np.abs(w0), np.abs(w1))[nz]).max()))
        for k in ("ts", "track", "label", "status", "forget"):
            differ |= set(a["idx"][a[k] != o[k]].tolist())
    return worst, sorted(differ)


def check_particles(sc, ref_sp, got, what, tol=None):
    """every slot but the time slots (the ring tests hold those) against a `particles` record: integers and positions
    exactly; weights bit for bit, or within tol (relative to the reference's)"""
    cfg = config(sc["variant"])
    _, s = dims(cfg)
    ref = rc.dense(cfg, ref_sp)
    keep = np.arange(len(ref["status"])) % s != 0
    for k in ("status", "ts", "track", "label", "forget"):
        bad = keep & (ref[k] != got[k])
        assert not bad.any(), "%s: %s differs at slots %s: reference %s, got %s" % (what, k, np.flatnonzero(bad)[:8], ref[k][bad][:8], got[k][bad][:8])
    for k in ("px", "py", "pz"):
        bad = keep & (bits(ref[k]) != bits(got[k]))
        assert not bad.any(), "%s: %s differs at slots %s: reference %s, got %s" % (what, k, np.flatnonzero(bad)[:8], ref[k][bad][:8], got[k][bad][:8])
    r, g = ref["w"].astype(np.float64), got["w"].astype(np.float64)
    rel = np.abs(r - g) / np.maximum(np.abs(r), 1e-30)
    if tol is None:
        bad = keep & (bits(ref["w"]) != bits(got["w"]))
    else:
        floor = float(np.spacing(np.abs(ref["w"][keep]).max()))          # one ulp of the largest magnitude in play
        assert tol <= ORDER_CAP
        bad = keep & ~(np.abs(r - g) <= np.maximum(tol * np.abs(r), floor))
        print("%s: largest relative weight difference %.3e, allowed %.3e" % (what, float(rel[keep & (r != 0)].max(initial=0.0)), tol))
    assert not bad.any(), "%s: weight differs at slots %s: reference %s, got %s (relative %s, allowed %s)" % (
        what, np.flatnonzero(bad)[:8], ref["w"][bad][:8], got["w"][bad][:8], rel[bad][:8], tol)


def owners_of_dump(st):
    own = {}
    for i in np.flatnonzero(st["owner"] != NO_TRACK):
        own.setdefault(int(st["owner"][i]), []).append(int(i))
    return own


def check_owners(ref_owners, got_dump, what):
    ref = {t: [int(i) for i in v] for t, v in ref_owners.items() if len(v)}        # the reference keeps emptied sets as keys
    got = owners_of_dump(got_dump)
    assert sorted(ref) == sorted(got), "%s: tracks with particles: reference %s, got %s" % (what, sorted(ref), sorted(got))
    for t in ref:
        assert ref[t] == got[t], "%s: owner set of track %d: reference %s, got %s" % (what, t, ref[t][:12], got[t][:12])


def check_births(sc, rec, m, what):
    """a map after the frame stopped after "birth" against the reference's answer: particles, noise cursor, owner sets,
    the number of particles added and of voxels resampled - all exact"""
    st = m.dump_state()
    check_particles(sc, ref_filter.first(rec, "particles", 1), st, what + " after the births")
    cursor = ref_filter.first(rec, "cursor")
    assert m.ring_state()["birth_cursor"] == cursor, "%s: noise cursor %d, reference %d" % (what, m.ring_state()["birth_cursor"], cursor)
    check_owners(ref_filter.first(rec, "owners"), st, what)
    births = ref_filter.first(rec, "births")
    stats = m.stats()
    assert stats["n_birth_success"] == births["added"], "%s: %d particles added, reference %d" % (what, stats["n_birth_success"], births["added"])
    assert stats["n_resampled_voxels"] == len(births["resampled"]), "%s: %d voxels resampled, reference %d" % (
        what, stats["n_resampled_voxels"], len(births["resampled"]))


def check_two_frames(sc, rec_a, rec_c, m, what):
    """after the second frame.  PINNED branch: the moved particles of one object that land in one voxel take its slots in
    the walk order of the object's set - std::unordered_set order in the reference, ascending index in the oracle and the
    library (as in move_overflow) - so in the voxels the object moved into, the rows are compared as a multiset per
    voxel, positions included, and the object's owner set by voxel; everything else slot by slot."""
    cfg = config(sc["variant"])
    _, s = dims(cfg)
    st = m.dump_state()
    ref_sp = ref_filter.first(rec_c, "particles", 3)       # after: weight 1, births 1, weight 2, births 2
    ref = rc.dense(cfg, ref_sp)
    track = sc["moved_track"]
    moved = ref_filter.first(rec_c, "move")[0]
    before = ref_filter.first(rec_a, "owners")[track]
    assert len(moved) == len(before) > 0 and not set(moved.tolist()) & set(before.tolist()), "the object did not move as a whole"
    assert (ref["status"][before] == INVALID).all() and (ref["track"][moved] == track).all()
    voxels = sorted(set(int(i) // s for i in moved))
    free = np.zeros(len(ref["status"]), bool)
    for v in voxels:
        free[v * s + 1:(v + 1) * s] = True
        rows = lambda d: sorted((int(bits(d["px"][i:i + 1])[0]), int(bits(d["py"][i:i + 1])[0]), int(bits(d["pz"][i:i + 1])[0]), int(bits(d["w"][i:i + 1])[0]),
                                 int(d["ts"][i]), int(d["track"][i]), int(d["label"][i]), int(d["status"][i]), int(d["forget"][i]))
                                for i in range(v * s + 1, (v + 1) * s) if d["status"][i] != INVALID)
        assert rows(ref) == rows(st), "%s: voxel %d after the move: reference %s, got %s" % (what, v, rows(ref), rows(st))
        assert np.array_equal(ref["status"][v * s:(v + 1) * s] != INVALID, st["status"][v * s:(v + 1) * s] != INVALID), "%s: voxel %d" % (what, v)
    masked = {k: np.where(free, ref[k], st[k]) for k in ("px", "py", "pz", "w", "ts", "track", "label", "status", "forget")}
    check_particles(sc, ref_sp, masked, what + " after the second frame")
    assert m.ring_state()["birth_cursor"] == ref_filter.first(rec_c, "cursor", 1), what
    ref_own = {t: [int(i) for i in v] for t, v in ref_filter.first(rec_c, "owners", 1).items() if len(v)}
    got_own = owners_of_dump(st)
    assert sorted(ref_own) == sorted(got_own), (sorted(ref_own), sorted(got_own))
    for t in ref_own:
        if t == track:
            assert sorted(i // s for i in ref_own[t]) == sorted(i // s for i in got_own[t]), "%s: owner set of the moved track" % what
        else:
            assert ref_own[t] == got_own[t], "%s: owner set of track %d" % (what, t)
    births = ref_filter.first(rec_c, "births", 1)
    assert births["added"] > 0 and m.stats()["n_birth_success"] == births["added"]
    want = 3 * sc["params"]["nb_ptc_num_per_point"] * (sum(1 for r in sc["cloud"] if r[8]) + sum(1 for r in sc["cloud2"] if r[8]))
    assert ref_filter.first(rec_c, "cursor", 1) == want, "the second frame does not go on from the first one's cursor"


# ------------------------------------------------------------------------------------------------ the scenarios hit their cases
def assert_weight_cases(sc, rec):
    """what the reference answered shows that a scenario exercises what its docstring says"""
    cfg = config(sc["variant"])
    name, sp = sc["name"], sc["state"]
    binned = np.sort(np.concatenate([v for v in ref_filter.first(rec, "bins").values()]))
    assert np.array_equal(binned, sp["idx"]), "%s: the visibility pass does not bin every particle" % name
    after = ref_filter.first(rec, "particles", 0)
    assert np.array_equal(after["idx"], sp["idx"]) and (after["status"] == UPDATED).all() and (after["ts"] == sc["ts"]).all()
    if name.startswith("weight_single"):
        assert len(ref_filter.first(rec, "bins")) == len(sp["idx"]), "two particles share a pixel"
        changed = bits(after["w"]) != bits(sp["w"])
        assert changed.all() and len(set(bits(after["w"] / sp["w"]).tolist())) >= 4, "the pairs do not differ"
    if name == "weight_window_edges":
        bins = ref_filter.first(rec, "bins")
        for r, c in sc["edge_pixels"] + [sc["invalid_holder"]]:
            assert len(bins.get(r * cfg["width"] + c, ())) == 3, "pixel (%d, %d) does not hold its three particles" % (r, c)
    if name.startswith("weight_forget"):
        pairs = set(zip(sp["forget"].tolist(), after["forget"].tolist()))
        if sc["params"]["if_use_independent_filter"]:
            assert all(a == b for a, b in pairs), pairs
        else:
            assert {(4, 5), (5, 5), (4, 0), (5, 0), (0, 1), (3, 0), (3, 4), (0, 0)} <= pairs, sorted(pairs)


def assert_birth_cases(sc, rec):
    cfg = config(sc["variant"])
    _, s = dims(cfg)
    births, after = ref_filter.first(rec, "births"), rc.dense(cfg, ref_filter.first(rec, "particles", 1))
    resampled = set(births["resampled"].tolist())
    prm = sc["params"]
    per_point = prm["nb_ptc_num_per_point"] if prm["if_consider_depth_noise"] else 1
    n_valid = sum(1 for row in sc["cloud"] if row[8])
    assert 0 < births["added"] < per_point * n_valid, "every insertion succeeded, or none"
    kinds = {}
    for v, kind in sc["voxels"]:
        status = after["status"][v * s + 1:(v + 1) * s]
        kinds.setdefault(kind, []).append((v in resampled, int((status == UPDATED).sum()), int((status == REGULAR_BORN).sum())))
    assert all(not r and u == 0 and b == s - 1 for r, u, b in kinds["empty"]), kinds["empty"]           # full of newborns, never resampled
    assert all(r and u == 0 and b > 0 for r, u, b in kinds["to_empty"]), kinds["to_empty"]              # emptied, then born into
    assert all(not r and u == s >> 1 and b == s - 1 - (s >> 1) for r, u, b in kinds["fills"]), kinds["fills"]
    assert all(r and b > 0 for r, u, b in kinds["full"] + kinds["full_static"] + kinds["heavy"]), kinds
    drawing = prm["if_consider_depth_noise"] and prm["nb_ptc_num_per_point"] != 1
    want = (sc["burn"] + 3 * per_point * n_valid) % GAUSSIAN_RANDOM_NUM if drawing else sc["burn"]
    assert ref_filter.first(rec, "cursor") == want, (ref_filter.first(rec, "cursor"), want)
    if sc["name"] == "cursor_wrap":
        assert want < sc["burn"], "the cursor does not cross the end of the table"
    own = {t: v for t, v in ref_filter.first(rec, "owners").items() if len(v)}
    assert {3, 4, 7} <= set(own) and all(t <= MAX_MOVABLE for t in own), sorted(own)
    before = len(owners_of(sc["state"])[7])
    assert 0 < len(own[7]) < before, "the resampling takes nothing out of the stored track's owner set"


def assert_resample_cases(sc, ref_sp):
    cfg = config(sc["variant"])
    _, s = dims(cfg)
    after, before = rc.dense(cfg, ref_sp), rc.dense(cfg, sc["state"])
    live = lambda st, v: [float(st["w"][i]) for i in range(v * s + 1, (v + 1) * s) if st["status"][i] == UPDATED]
    v = sc["voxels"]
    assert live(after, v[0]) == live(before, v[0])                                   # S/2: untouched
    assert live(after, v[2]) == [] and len(live(after, v[3])) > 0                    # just below 0.01: emptied; just above: resampled
    assert set(live(after, v[4])) == {1.0}                                           # clipped at 1
    assert 0 < len(live(after, v[5])) <= s >> 1 and len(live(after, v[5])) < len(live(before, v[5]))   # the light ones before the heavy one go
    if len(v) > 8:
        keep = lambda st, x: [int(st["status"][i]) for i in range(x * s + 1, (x + 1) * s) if st["status"][i] not in (UPDATED, INVALID)]
        assert keep(after, v[8]) == keep(before, v[8]) == [COPIED] and keep(after, v[9]) == [REGULAR_BORN, GUESSED_BORN]
