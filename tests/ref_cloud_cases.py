"""Scenarios for the reference's generateLabeledPointCloud / manualResize (utils/pointcloud_tools.h:88-310, 1104-1133),
the comparison rules, and the adapters that feed the same scenario to the CPU oracle and to the HIP library.

Plain numpy, importable without a GPU.  Inputs are regenerated from seeds; tests/golden/ref_cloud_<variant>.npz holds
only what oracle/ref_cloud_harness.cpp - the reference's own function compiled over oracle/ref_shims/ - answered, plus
a hash of the scenario file it was given.  Everything the oracle and the library are configured with (camera, depth
range, largest movable id, Sky's instance, the label -> instance table, the label id of an entry's label) is read from
that record, never from the project's constants; only T0's grid (which the function does not read) is the project's.

Every image is built at the configured size (128 x 80) with about 1,000 to 2,000 valid depth pixels, NaN elsewhere: the
corners, first and last row and column, pixel indices around multiples of the launch's block size (256) and in the last
block, and both sides of every mask edge.  For the BOOST variants it is then spread over the sensor-size image, to the
source pixels that manualResize reads; every other source pixel holds a decoy (a valid depth, another mask value), so
that an implementation that reads another source pixel gets other points.

Comparison rules (compare()):
  * is_valid, track id, label id and the reduced depth image: exact, everywhere;
  * sigma: bit for bit (one float multiply and one add, contraction off on both sides);
  * what the reference leaves unset is not compared but must hold the library's pinned values: an invalid point is all
    zero with sigma = zero-order term (0.1f without the noise flag); a point the box filter clipped has the noise
    model's sigma;
  * position, exact scenarios (quaternion of 0, +-1, +-0.5, position in quarters, depth in eighths, f and c powers of
    two: every intermediate is exact in double, so any correct double formula gives the same bits): bit for bit;
  * position, other scenarios: both sides round one double to float.  Two correct double evaluations differ by a few
    units of 2^-53 relative (the inverse intrinsics as 1/f or through the cofactors, the order of the three-term sums),
    the float grid is 2^-24 relative, so a coordinate straddles a rounding boundary with probability of the order
    2^-26.  Hence: no coordinate further than the adjacent float, and adjacent floats in at most AMBIGUOUS_CAP of a
    scenario's coordinates.  The cap comes from that reasoning, not from a measurement; at these scenario sizes
    (at most 6,000 coordinates) it allows no differing coordinate at all.
"""
import hashlib

import numpy as np

from semantic_dsp_map_amd import synth

W, H = 128, 80
TPB = 256                       # threads per block of the two kernels
AMBIGUOUS_CAP = 1e-4            # share of a scenario's coordinates that may be the adjacent float
MAX_CLOUD_OBJECTS = 64          # sdm_scratch.h
SENSOR = {"zed2": (256, 160, 0.5), "third": (427, 267, 0.3), "plain": (W, H, 1.0), "static": (W, H, 1.0)}   # width, height, rescale
# the cameras the variants' sed files produce, only to design inputs with (the tests read the record)
_f32 = np.float32
DESIGN_CAMERA = {"zed2": (80.0, 80.0, 64.0, 40.0), "plain": (64.0, 64.0, 64.0, 40.0), "static": (80.0, 80.0, 64.0, 40.0),
                 "third": tuple(float(_f32(0.3) * _f32(v)) for v in (321.13, 312.87, 210.71, 136.29))}
DESIGN_DEPTH = (float(_f32(0.3)), 12.0)
WIDE = np.array([[-500.0, -500.0, -500.0], [500.0, 500.0, 500.0]])   # key points whose box holds every point
STATIC_NAMED = np.array([1, 3, 4, 5, 6, 7, 8, 9, 10, 11], np.uint8)    # mask values of labels with a static instance, Sky left out
STATIC_SKY = 2
STATIC_TO_ZERO = np.array([0, 12, 13, 14, 15, 100, 254, 255], np.uint8)  # values whose label has no name or no static instance

NAMES = {
    "zed2": ["track_label", "static_movable", "static_movable_clipped", "zero_objects", "boundary_id", "depth_edges", "derived_box",
             "sky_and_255"],
    "third": ["resize_rows", "overlap_ab", "overlap_ba", "max_objects", "no_static", "noise_flag_off"],
    "plain": ["exact_axis", "exact_half", "plain_static_movable", "plain_boundary"],
    "static": ["instances_off", "instances_off_no_static", "depth_edges_plain"],
}


# ------------------------------------------------------------------ the reference's arithmetic, restated to design inputs
def source_index(n_dst, n_src, scale):
    """manualResize (:1119-1128): min(int(i * (1.f / scale)), n_src - 1), the product in float"""
    inv = _f32(1.0) / _f32(scale)
    return np.minimum((np.arange(n_dst).astype(np.float32) * inv).astype(np.int64), n_src - 1)


def rotation(q, dtype=np.float64):
    """Eigen's Quaternion::toRotationMatrix"""
    w, x, y, z = (dtype(v) for v in q)
    two = dtype(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = dtype(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], dtype)


def backproject(depth, camera, pose, dtype=np.float64):
    """:243-249 for every pixel of an H x W depth image, in `dtype` throughout -> (H, W, 3) of that dtype"""
    fx, fy, cx, cy = (dtype(v) for v in camera[:4])
    d = np.asarray(depth).astype(dtype)
    j, i = np.meshgrid(np.arange(d.shape[1]).astype(dtype), np.arange(d.shape[0]).astype(dtype))
    one = dtype(1)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z = (one / fx * j + -cx / fx) * d, (one / fy * i + -cy / fy) * d, d
        r = rotation(pose[3:], dtype)
        t = [dtype(v) for v in pose[:3]]
        return np.stack([((r[a, 0] * x + r[a, 1] * y) + r[a, 2] * z) + t[a] for a in range(3)], axis=-1)


def box_rule(kpts):
    """:180-199: min starts at the largest double, max at the SMALLEST POSITIVE double, then +- 1 m -> 6 doubles
    (min x, max x, min y, max y, min z, max z)"""
    lo = np.full(3, np.finfo(np.float64).max)
    hi = np.full(3, np.finfo(np.float64).tiny)
    for p in np.asarray(kpts, np.float64).reshape(-1, 3):
        lo = np.where(p < lo, p, lo)
        hi = np.where(p > hi, p, hi)
    return np.stack([lo - 1.0, hi + 1.0], axis=1).reshape(-1)


# ------------------------------------------------------------------ building blocks
def pick(rng, n):
    """an H x W boolean image of about n pixels that get a valid depth"""
    m = np.zeros(H * W, bool)
    m[[0, W - 1, (H - 1) * W, H * W - 1]] = True
    m[rng.choice(W, 12, replace=False)] = True
    m[(H - 1) * W + rng.choice(W, 12, replace=False)] = True
    m[rng.choice(H, 8, replace=False) * W] = True
    m[rng.choice(H, 8, replace=False) * W + W - 1] = True
    for k in (1, 2, 7, 20, 39):
        m[k * TPB - 2:k * TPB + 2] = True
    m[H * W - TPB:H * W - TPB + 6] = True
    m[rng.choice(H * W, n, replace=False)] = True
    return m.reshape(H, W)


def rect(r0, r1, c0, c1, value=1):
    m = np.zeros((H, W), np.uint8)
    m[r0:r1, c0:c1] = value
    return m


def edge_pixels(mask, rng, share=0.5):
    """pixels on both sides of a mask's edge, thinned"""
    on = mask > 0
    e = np.zeros_like(on)
    e[:, 1:] |= on[:, 1:] != on[:, :-1]
    e[:, :-1] |= on[:, 1:] != on[:, :-1]
    e[1:, :] |= on[1:, :] != on[:-1, :]
    e[:-1, :] |= on[1:, :] != on[:-1, :]
    return e & (rng.random((H, W)) < share)


def random_depth(rng, where, lo=0.6, hi=11.0):
    d = np.full((H, W), np.nan, np.float32)
    d[where] = rng.uniform(lo, hi, int(where.sum())).astype(np.float32)
    return d


def static_background(rng):
    return STATIC_NAMED[rng.integers(0, len(STATIC_NAMED), (H, W))]


def tilted_pose(rng, reach=40.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.concatenate([rng.uniform(0.4, 1.0, 3) * reach * rng.choice([-1.0, 1.0], 3), q])


def points_of(variant, depth, pose, mask):
    """double-precision positions of the valid pixels under a mask, to take key points from"""
    p = backproject(depth, DESIGN_CAMERA[variant], pose)
    return p[(mask > 0) & np.isfinite(depth)]


def finish(variant, name, depth, static, objects, pose, noise, exact=False, static_at=0):
    """objects: [(track, label word, key points, H x W mask)].  Spreads the images over the sensor's size."""
    sw, sh, scale = SENSOR[variant]
    seed = int(hashlib.sha256(("%s/%s" % (variant, name)).encode()).hexdigest()[:8], 16)
    rng = np.random.default_rng(seed)

    def spread(img, decoy):
        if (sw, sh) == (W, H):
            return np.ascontiguousarray(img)
        out = decoy.astype(img.dtype)
        out[np.ix_(source_index(H, sh, scale), source_index(W, sw, scale))] = img
        return out

    rr, cc = np.meshgrid(np.arange(sh), np.arange(sw), indexing="ij")
    blocks = (((rr + cc // 16) % 2) * 255).astype(np.uint8)    # a mask decoy that changes with every row and every 16 columns
    entries = [dict(track=int(t), label=l, kpts=np.asarray(k, np.float64).reshape(-1, 3), mask=spread(m, blocks)) for t, l, k, m in objects]
    if static is not None:
        entries.insert(static_at, dict(track=0, label="static", kpts=np.zeros((0, 3)),
                                       mask=spread(static, rng.integers(0, 16, (sh, sw)).astype(np.uint8))))
    return dict(variant=variant, name=name, exact=exact, noise=noise, pose=np.asarray(pose, np.float64),
                depth=spread(depth, rng.uniform(1.0, 11.0, (sh, sw)).astype(np.float32)), entries=entries,
                dst=dict(depth=depth, static=static, objects=objects))


# ------------------------------------------------------------------ the scenarios
def _rng(variant, name):
    return np.random.default_rng(int(hashlib.sha256(("seed/%s/%s" % (variant, name)).encode()).hexdigest()[:8], 16))


def _movable_static(rng):
    """a static mask with patches whose value names no static instance (the reference makes them movable id 0)"""
    s = static_background(rng)
    for k, v in enumerate(STATIC_TO_ZERO):
        s[4 + 9 * k:11 + 9 * k, 10:70] = v
    return s


def scenario(variant, name):
    rng = _rng(variant, name)
    on = (True, 0.02, 0.3)          # the noise flag with a non-zero first-order term
    if name == "track_label":       # item 2: two entries with one track id and different labels
        a, c, d = rect(5, 30, 8, 50), rect(40, 70, 20, 70), rect(55, 78, 60, 110)
        where = pick(rng, 300) | edge_pixels(a, rng) | edge_pixels(c, rng) | edge_pixels(d, rng) | ((a | c | d) > 0) & (rng.random((H, W)) < 0.08)
        objects = [(7, "Car", WIDE, a), (7, "Person", WIDE, rect(0, 0, 0, 0)), (9, "Truck", WIDE, c), (9, "Car", WIDE, d)]
        return finish(variant, name, random_depth(rng, where), static_background(rng), objects, tilted_pose(rng, 3.0), on, static_at=2)
    if name in ("static_movable", "static_movable_clipped", "zero_objects", "plain_static_movable", "instances_off"):   # item 3
        s = _movable_static(rng)
        o0, o5 = rect(30, 50, 80, 120), rect(60, 75, 75, 125)
        where = pick(rng, 300) | np.isin(s, STATIC_TO_ZERO) & (rng.random((H, W)) < 0.12)
        where |= edge_pixels(o0, rng) | edge_pixels(o5, rng)
        objects = {"static_movable": [(5, "Car", WIDE, o5), (0, "Person", WIDE, o0)], "plain_static_movable": [(0, "Truck", WIDE, o0), (5, "Car", WIDE, o5)],
                   "static_movable_clipped": [(5, "Car", WIDE, o5), (3, "Person", WIDE, o0)], "zero_objects": [],
                   "instances_off": [(0, "Person", WIDE, o0), (5, "Car", WIDE, o5)]}[name]
        return finish(variant, name, random_depth(rng, where), s, objects, tilted_pose(rng, 20.0), on)
    if name in ("boundary_id", "plain_boundary"):   # item 4: a track id equal to the largest movable id, and its neighbour below
        a, b, c = rect(10, 40, 10, 60), rect(30, 70, 50, 110), rect(60, 78, 5, 40)
        where = pick(rng, 300) | edge_pixels(a, rng) | edge_pixels(b, rng) | edge_pixels(c, rng) | ((a | b | c) > 0) & (rng.random((H, W)) < 0.07)
        far = np.array([[900.0, 900.0, 900.0], [901.0, 901.0, 901.0]])   # a box no point of the frame is inside
        objects = [(65523, "Car", far, a), (65522, "Person", far, b), (11, "Truck", WIDE, c)]
        return finish(variant, name, random_depth(rng, where), static_background(rng), objects, tilted_pose(rng, 10.0),
                      on if variant == "zed2" else (False, 0.02, 0.3))
    if name in ("depth_edges", "depth_edges_plain"):   # item 5: strict comparisons of the float promoted to double
        lo, hi = (_f32(v) for v in DESIGN_DEPTH)
        inf = _f32(np.inf)
        specials = np.array([lo, np.nextafter(lo, -inf), np.nextafter(lo, inf), hi, np.nextafter(hi, -inf), np.nextafter(hi, inf), inf, -inf,
                             0.0, -0.0, -1.0, 1e-42, -1e-42, np.finfo(np.float32).tiny, np.finfo(np.float32).max, 0.29999, 12.00001], np.float32)
        where = pick(rng, 700)
        depth = random_depth(rng, where)
        flat = depth.reshape(-1)
        at = np.flatnonzero(where.reshape(-1))
        flat[at[::2]] = specials[np.arange(len(at[::2])) % len(specials)]     # every second valid pixel, block borders included
        a = rect(20, 60, 30, 100)
        objects = [(4, "Car", WIDE, a)]
        return finish(variant, name, depth, static_background(rng), objects, tilted_pose(rng, 5.0), on if variant == "zed2" else (False, 0.05, 0.2))
    if name == "derived_box":       # item 6: the box's max starts at the smallest positive double
        pose = np.array([-2.5, -1.5, -4.0, 1.0, 0.0, 0.0, 0.0])
        neg, empty, part = rect(5, 75, 70, 125), rect(5, 40, 5, 40), rect(45, 78, 5, 60)
        where = pick(rng, 300) | edge_pixels(neg, rng, 0.3) | ((neg | empty | part) > 0) & (rng.random((H, W)) < 0.12)
        depth = random_depth(rng, where, 0.5, 6.0)
        kp_part = points_of(variant, depth, pose, part)[:4]
        kp_neg = np.array([[-3.0, -2.0, -2.5], [-2.0, -1.5, -1.0]])   # all negative: the recorded max stays at DBL_MIN, so hi = 1.0
        objects = [(21, "Car", kp_neg, neg), (22, "Person", np.zeros((0, 3)), empty), (23, "Truck", kp_part, part)]
        return finish(variant, name, depth, static_background(rng), objects, pose, on)
    if name == "sky_and_255":
        s = static_background(rng)
        s[0:30, :] = STATIC_SKY
        s[60:80, 0:64] = 255
        a = rect(20, 45, 40, 90)      # an object over Sky pixels and over named ones
        where = pick(rng, 600) | edge_pixels(a, rng) | edge_pixels(s == STATIC_SKY, rng, 0.3)
        objects = [(2, "Person", WIDE, a)]
        return finish(variant, name, random_depth(rng, where), s, objects, tilted_pose(rng, 8.0), on)
    if name in ("resize_rows", "noise_flag_off"):   # item 1: int(i * (1.f / 0.3f)); a tilted pose tens of metres out
        a, b = rect(10, 50, 20, 80), rect(35, 75, 60, 120)
        where = pick(rng, 1500) | edge_pixels(a, rng) | edge_pixels(b, rng)
        depth = random_depth(rng, where)
        pose = tilted_pose(rng, 60.0)
        objects = [(1, "Car", points_of(variant, depth, pose, a)[:2], a), (2, "Person", WIDE, b)]
        return finish(variant, name, depth, static_background(rng), objects, pose, on if name == "resize_rows" else (False, 0.03, 0.25))
    if name in ("overlap_ab", "overlap_ba"):        # the later entry wins, whichever it is
        a, b = rect(10, 55, 15, 85), rect(30, 75, 50, 120)
        rng = _rng(variant, "overlap")              # the same inputs for both orders
        where = pick(rng, 500) | edge_pixels(a, rng) | edge_pixels(b, rng) | ((a & b) > 0) & (rng.random((H, W)) < 0.3)
        depth, s, pose = random_depth(rng, where), static_background(rng), tilted_pose(rng, 30.0)
        objects = [(31, "Car", WIDE, a), (32, "Person", WIDE, b * 200)]
        return finish(variant, name, depth, s, objects if name == "overlap_ab" else objects[::-1], pose, on)
    if name == "max_objects":       # MAX_CLOUD_OBJECTS objects, 16 x 10 pixels each, every one overlapping the next
        where = pick(rng, 1200)
        depth, pose = random_depth(rng, where), tilted_pose(rng, 25.0)
        objects = []
        for k in range(MAX_CLOUD_OBJECTS):
            r0, c0 = (k // 8) * 10, (k % 8) * 16
            m = rect(r0, min(r0 + 12, H), c0, min(c0 + 19, W))
            objects.append((100 + k, ("Car", "Person", "Truck")[k % 3], WIDE if k % 4 else points_of(variant, depth, pose, m)[:3], m))
        return finish(variant, name, depth, static_background(rng), objects, pose, on)
    if name in ("no_static", "instances_off_no_static"):
        a, b = rect(10, 50, 20, 80), rect(35, 75, 60, 120)
        where = pick(rng, 800) | edge_pixels(a, rng) | edge_pixels(b, rng)
        depth, pose = random_depth(rng, where), tilted_pose(rng, 15.0)
        objects = [(1, "Car", points_of(variant, depth, pose, a)[:3], a), (2, "Person", WIDE, b)]
        return finish(variant, name, depth, None, objects, pose, on)
    if name in ("exact_axis", "exact_half"):
        q = [0.0, 0.0, 1.0, 0.0] if name == "exact_axis" else [0.5, -0.5, 0.5, -0.5]
        pose = np.array([12.25, -3.5, 40.75] + q)
        a = rect(20, 60, 30, 100)
        where = pick(rng, 1200) | edge_pixels(a, rng)
        depth = np.full((H, W), np.nan, np.float32)
        depth[where] = (rng.integers(3, 96, int(where.sum())) / 8.0).astype(np.float32)
        return finish(variant, name, depth, static_background(rng), [(6, "Car", WIDE, a)], pose, (name == "exact_axis", 0.02, 0.3), exact=True)
    raise KeyError(name)


def scenarios(variant):
    return [scenario(variant, n) for n in NAMES[variant]]


def inputs_hash(script_text):
    return np.frombuffer(hashlib.sha256(script_text.encode("ascii")).digest(), np.uint8).copy()


# ------------------------------------------------------------------ feeding the oracle and the library from the record
def map_config(rec):
    """T0's grid with the recorded image, camera, depth range and largest movable id"""
    cam = rec["camera"]
    cfg = dict(synth.CONFIGS["T0"])
    cfg.update(width=int(rec["variant"][3]), height=int(rec["variant"][4]), fx=float(cam[0]), fy=float(cam[1]), cx=float(cam[2]),
               cy=float(cam[3]), depth_min=float(cam[4]), depth_max=float(cam[5]), max_movable_track=int(rec["max_movable"][0]))
    return cfg


def map_params(sc):
    flag, first, zero = sc["noise"]
    return dict(synth.PARAMS["vkitti2"], if_consider_depth_noise=1 if flag else 0, depth_noise_first_order=first, depth_noise_zero_order=zero)


def raw_arguments(sc, rec):
    """what sdm_update_raw_ex / generate_cloud_ex get for a scenario: a dict of keyword-free values"""
    setting, boost, consider = (int(v) for v in rec["variant"][:3])
    sw, sh, _ = SENSOR[sc["variant"]]
    static, objects, boxes = None, [], []
    for e, label in zip(sc["entries"], rec["entry_labels"]):
        if e["label"] == "static":
            if static is None:
                static = e["mask"]
            continue
        objects.append((e["track"], max(int(label), 0), e["mask"]))   # a label without a name: the lookup's default, 0
        boxes.append(box_rule(e["kpts"]))
    zed2 = setting == 3
    return dict(depth=sc["depth"], static=static, table=rec["label_to_instance"][:256].astype(np.uint16), objects=objects,
                pos=sc["pose"][:3], q=sc["pose"][3:], consider_instance=bool(consider), src_size=(sw, sh) if boost else None,
                rescale=float(rec["camera"][6]), sky_instance=int(rec["sky"][0]) if zed2 else -1,
                object_bbox=np.array(boxes if boxes else [[0.0] * 6], np.float64).reshape(-1, 6) if zed2 else None)


def oracle_cloud(make, sc, rec):
    """make(cfg, params) -> OracleMap.  Returns (LabeledPoint image, reduced depth)."""
    a = raw_arguments(sc, rec)
    m = make(dict(map_config(rec), bin_order=1), map_params(sc))
    return m.generate_cloud_ex(a["depth"], a["static"], a["table"], a["objects"], a["pos"], a["q"], a["consider_instance"],
                               src_size=a["src_size"], rescale=a["rescale"], sky_instance=a["sky_instance"], object_bbox=a["object_bbox"])


# ------------------------------------------------------------------ comparison
def float_steps(a, b):
    """distance in representable floats between two float32 arrays of finite values"""
    def key(x):
        u = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7fffffff), u)
    return np.abs(key(a) - key(b))


def position_report(ref_pos, got_pos):
    """(largest distance in floats, share of coordinates that differ)"""
    steps = float_steps(ref_pos, got_pos)
    return (int(steps.max()) if steps.size else 0), (float((steps > 0).mean()) if steps.size else 0.0)


def check_positions(ref_pos, got_pos, exact, tag):
    worst, share = position_report(ref_pos, got_pos)
    if exact:
        assert worst == 0, "%s: positions of an exact scenario differ by up to %d floats" % (tag, worst)
    else:
        assert worst <= 1, "%s: a coordinate is %d floats away from the reference's" % (tag, worst)
        assert share <= AMBIGUOUS_CAP, "%s: %.4f %% of the coordinates are the adjacent float (cap %.4f %%)" % (tag, 100 * share, 100 * AMBIGUOUS_CAP)


def compare(sc, rec, cloud, depth, tag):
    """cloud: LabeledPoint image (H*W), depth: the reduced depth image the oracle / library used, or None"""
    tag = "%s/%s %s" % (sc["variant"], sc["name"], tag)
    n = H * W
    cloud = cloud.reshape(-1)
    assert cloud.size == n
    if depth is not None:
        assert np.array_equal(np.asarray(depth, np.float32).reshape(-1).view(np.uint32), rec["depth"].reshape(-1).view(np.uint32)), tag + ": reduced depth"
    valid = np.zeros(n, bool)
    valid[rec["pixel"]] = True
    assert np.array_equal(cloud["is_valid"] > 0, valid), "%s: is_valid differs at pixels %s" % (tag, np.flatnonzero((cloud["is_valid"] > 0) != valid)[:8])
    got = cloud[rec["pixel"]]
    bad = np.flatnonzero(got["track_id"] != rec["track"])
    assert bad.size == 0, "%s: track id at pixels %s: %s, reference %s" % (tag, rec["pixel"][bad[:6]], got["track_id"][bad[:6]], rec["track"][bad[:6]])
    bad = np.flatnonzero(got["label_id"] != rec["label"])
    assert bad.size == 0, "%s: label id at pixels %s: %s, reference %s" % (tag, rec["pixel"][bad[:6]], got["label_id"][bad[:6]], rec["label"][bad[:6]])
    flag, first, zero = sc["noise"]
    dv = rec["depth"].reshape(-1)[rec["pixel"]]
    model = (_f32(zero) + _f32(first) * dv).astype(np.float32) if flag else np.full(len(dv), 0.1, np.float32)
    kept = rec["clipped"] == 0
    assert np.array_equal(got["sigma"][kept].view(np.uint32), rec["sigma"][kept].view(np.uint32)), tag + ": sigma"
    assert np.array_equal(got["sigma"][~kept].view(np.uint32), model[~kept].view(np.uint32)), tag + ": sigma of a clipped point (pinned: the noise model's)"
    rest = cloud[~valid]
    for k in ("x", "y", "z", "track_id", "label_id"):
        assert not rest[k].any(), "%s: %s of an invalid point (pinned: zero)" % (tag, k)
    assert np.all(rest["sigma"] == (_f32(zero) if flag else _f32(0.1))), tag + ": sigma of an invalid point (pinned: the zero-order term)"
    check_positions(rec["pos"], np.stack([got["x"], got["y"], got["z"]], axis=1), sc["exact"], tag)


# ------------------------------------------------------------------ what each scenario must reach
def merged_ids(sc, rec):
    """the track-id image before the filters (:116-215), from the images at the configured size and the recorded tables"""
    dst = sc["dst"]
    ids = np.full((H, W), 65535, np.int64)
    if dst["static"] is not None:
        ids = rec["label_to_instance"][dst["static"].astype(np.int64) + 1]
    if rec["variant"][2]:
        for t, _, _, m in dst["objects"]:
            ids = np.where(m > 0, t, ids)
    return ids


def design_valid(sc):
    lo, hi = DESIGN_DEPTH
    d = sc["dst"]["depth"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(d) | (d < lo) | (d > hi))


def check_hits(sc, rec):
    """assert that the recorded answer of a scenario contains the case the scenario was written for"""
    name, variant = sc["name"], sc["variant"]
    ids = merged_ids(sc, rec).reshape(-1)
    px = rec["pixel"]
    mx = int(rec["max_movable"][0])
    setting = int(rec["variant"][0])
    pre = ids[px]                       # id before the box filter
    clipped = rec["clipped"] > 0
    ok = design_valid(sc).reshape(-1)
    if setting == 3:
        ok &= ids != int(rec["sky"][0])
    assert np.array_equal(np.flatnonzero(ok), px), "the valid pixels are not the designed ones"
    assert 300 <= len(px) <= 2600, len(px)
    for b in (0, W - 1, (H - 1) * W, TPB - 1, TPB, 39 * TPB):
        assert b in px or not ok[b]
    labels = dict(zip(rec["track_to_label"][:, 0].tolist(), rec["track_to_label"][:, 1].tolist()))
    objects = sc["dst"]["objects"]
    if name == "track_label":
        last_cover = np.zeros(H * W, np.int64)
        object_labels = [int(l) for l, e in zip(rec["entry_labels"], sc["entries"]) if e["label"] != "static"]
        for (_, _, _, m), label in zip(objects, object_labels):   # the label of the last mask that covers the pixel
            last_cover = np.where(m.reshape(-1) > 0, label, last_cover)
        differ = (pre <= mx) & (last_cover[px] != rec["label"])
        assert differ.sum() > 50 and labels == {7: 15, 9: 14}
    elif name in ("static_movable", "plain_static_movable"):
        from_static = (pre == 0) & np.isin(sc["dst"]["static"].reshape(-1)[px], STATIC_TO_ZERO)
        assert from_static.sum() > 200 and np.all(rec["track"][from_static] == 0) and np.all(rec["label"][from_static] == labels[0]) and labels[0] in (13, 15)
        for v in STATIC_TO_ZERO:
            assert np.any(sc["dst"]["static"].reshape(-1)[px][from_static] == v), v
    elif name in ("static_movable_clipped", "zero_objects"):
        from_static = (pre == 0)
        assert from_static.sum() > 200 and np.all(clipped[from_static]) and np.all(rec["track"][from_static] == 65535)
        assert (name == "zero_objects") == (len(objects) == 0) and 0 not in labels
    elif name == "instances_off":
        assert labels == {0: 0} and np.all(rec["label"][pre == 0] == 0)     # (the lookup of id 0 inserted it) and (pre == 0).sum() > 200 and not np.isin(rec["track"], [5]).any()
    elif name in ("boundary_id", "plain_boundary"):
        at_max = rec["track"] == mx
        assert mx == 65523 and at_max.sum() > 50 and np.all(rec["label"][at_max] == 14) and not clipped[at_max].any()
        below = pre == mx - 1
        assert below.sum() > 50 and (np.all(clipped[below]) if setting == 3 else np.all(rec["label"][below] == 15))
    elif name in ("depth_edges", "depth_edges_plain"):
        lo, hi = (_f32(v) for v in DESIGN_DEPTH)
        d = sc["dst"]["depth"].reshape(-1)
        inf = _f32(np.inf)
        for v, want in ((lo, True), (hi, True), (np.nextafter(lo, inf), True), (np.nextafter(hi, -inf), True), (np.nextafter(lo, -inf), False),
                        (np.nextafter(hi, inf), False), (inf, False), (-inf, False), (_f32(0), False), (_f32(-1), False), (_f32(1e-42), False)):
            at = np.flatnonzero(d == v)
            assert at.size >= 5 and np.all(np.isin(at, px) == (want and (setting != 3 or ids[at] != int(rec["sky"][0])))), v
        assert np.array_equal(rec["camera"][4:6], np.array([lo, hi], np.float32))
    elif name == "derived_box":
        pos = rec["pos"].astype(np.float64)
        neg, empty, part = (pre == 21), (pre == 22), (pre == 23)
        beyond = neg & ~clipped & (pos[:, 0] > -2.0 + 1.0 + 1e-3)      # kept although past the key points' max + 1 m: hi is 1.0
        assert beyond.sum() > 10 and np.all(pos[neg & ~clipped] < 1.0 + 1e-6) and (neg & clipped).sum() > 10
        assert empty.sum() > 50 and np.all(clipped[empty])
        assert (part & clipped).sum() > 10 and (part & ~clipped).sum() > 10
    elif name == "sky_and_255":
        s = sc["dst"]["static"].reshape(-1)
        over_sky = (s[px] == STATIC_SKY)
        assert over_sky.sum() > 20 and np.all(rec["track"][over_sky] == 2) and (design_valid(sc).reshape(-1) & (ids == int(rec["sky"][0]))).sum() > 50
        assert ((s[px] == 255) & clipped).sum() > 20
    elif name in ("resize_rows", "noise_flag_off"):
        sw, sh, scale = SENSOR[variant]
        rows = source_index(H, sh, scale)
        exact_rows = np.floor(np.arange(H) / np.float64(_f32(scale)))    # floor(i / scale) without the float product's rounding
        assert (rows != exact_rows).sum() >= 20 and rows.max() < sh - 1 and source_index(W, sw, scale).max() < sw - 1
        assert np.any(np.isin(px // W, np.flatnonzero(rows != exact_rows)))
        assert (clipped.sum() > 0 or name != "resize_rows") and (name == "resize_rows") == bool(sc["noise"][0]) and sc["noise"][1] != 0
        assert np.abs(sc["pose"][:3]).max() > 20
    elif name in ("overlap_ab", "overlap_ba"):
        a, b = (objects[0][3].reshape(-1) > 0), (objects[1][3].reshape(-1) > 0)
        both = (a & b)[px]
        assert both.sum() > 50 and np.all(rec["track"][both] == objects[1][0]) and objects[1][0] == (32 if name == "overlap_ab" else 31)
    elif name == "max_objects":
        assert len(objects) == MAX_CLOUD_OBJECTS and len(np.unique(rec["track"][rec["track"] <= mx])) >= 60 and clipped.sum() > 0
    elif name in ("no_static", "instances_off_no_static"):
        assert all(e["label"] != "static" for e in sc["entries"])
        bg = (rec["track"] == 65535) & ~clipped
        assert bg.sum() > 100 and np.all(rec["label"][bg] == 0)
        assert (clipped.sum() > 0) if setting == 3 else (len(labels) == 0 and np.all(rec["track"] == 65535))
    elif name in ("exact_axis", "exact_half"):
        assert sc["exact"] and np.all(np.isin(np.abs(sc["pose"][3:]), [0.0, 0.5, 1.0])) and np.all(sc["pose"][:3] * 4 == np.round(sc["pose"][:3] * 4))
        d = sc["dst"]["depth"].reshape(-1)[px]
        assert np.all(d * 8 == np.round(d * 8)) and np.array_equal(rec["camera"][:4], np.array([64, 64, 64, 40], np.float32))
    else:
        raise KeyError(name)
