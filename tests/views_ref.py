"""NumPy restatement of view scoring (include/sdm.h: sdm_query_views), for the tests, on top of tests/query_ref.py.

The rays of a view are built in float32 by the formula the header pins (R(q) as tests/shape_cases.py::quat_mat spells it
out, R d summed left to right, then * range, + pos: one IEEE operation at a time), every ray is walked by
query_ref.query_segments(record=True), and the distinct counts of a view come from the union of its rays' walks.
unambiguous_rays draws a ray table on which no view has a ray with two crossings within rounding of each other, so that
a comparison against this restatement never has to excuse a ray."""
import numpy as np

from semantic_dsp_map_amd import binding
from tests import query_ref as qr

F = np.float32


def rotation(q):
    """quat_mat in float32, entry by entry: q (n, 4) as (w, x, y, z) -> (n, 3, 3)"""
    q = np.asarray(q, F).reshape(-1, 4)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = F(1), F(2)
    with np.errstate(invalid="ignore", over="ignore"):
        R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                      two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                      two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=1)
    assert R.dtype == F
    return R.reshape(-1, 3, 3)


def rays_of(views, dirs):
    """-> a, b (n_views, n_rays, 3) float32 and given (n_views, n_rays): False where the view or the ray's vector has a
    non-finite number (a and b are NaN there: such a ray visits nothing)"""
    views = np.asarray(views, binding.VIEW).reshape(-1)
    d = np.asarray(dirs, F).reshape(-1, 3)
    R = rotation(views["q"])
    pos, rng = views["pos"].astype(F), views["range"].astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        rd = np.stack([(R[:, None, i, 0] * d[None, :, 0] + R[:, None, i, 1] * d[None, :, 1]) + R[:, None, i, 2] * d[None, :, 2]
                       for i in range(3)], axis=2)
        b = pos[:, None, :] + rng[:, None, None] * rd
    assert rd.dtype == F and b.dtype == F
    a = np.broadcast_to(pos[:, None, :], b.shape).copy()
    with np.errstate(invalid="ignore"):
        b = np.where((rng > 0)[:, None, None], b, a)   # range <= 0: the zero-length segment
    view_ok = np.isfinite(pos).all(axis=1) & np.isfinite(views["q"]).all(axis=1) & np.isfinite(rng)
    given = view_ok[:, None] & np.isfinite(d).all(axis=1)[None, :]
    a[~given], b[~given] = np.nan, np.nan
    return a, b, given


def query_views(geo, voxels, views, dirs):
    """-> (gain: VIEW_GAIN array, rays: SEGMENT_HIT-like dict of (n_views, n_rays) arrays, ray_unknown (n_views, n_rays))"""
    a, b, _ = rays_of(views, dirs)
    nv, nr = a.shape[:2]
    hits, walks = qr.query_segments(geo, voxels, a.reshape(-1, 3), b.reshape(-1, 3), record=True)
    occ = voxels["occ"]
    gain = np.zeros(nv, binding.VIEW_GAIN)
    unk = np.zeros((nv, nr), np.int32)
    for v in range(nv):
        seen = []
        for r in range(nr):
            w = walks[v * nr + r]
            assert len(w) == hits["cells"][v * nr + r]
            if w:
                o = occ[geo.voxel(np.array(w, np.int64))]
                unk[v, r] = int((o == -1).sum())
                assert (o[:-1] < 1).all()    # only the last cell of a walk can block
                seen.extend(w)
        g = gain[v]
        if seen:
            cells = np.unique(np.array(seen, np.int64), axis=0)
            o = occ[geo.voxel(cells)]
            g["n_unknown"], g["n_free"], g["n_occupied"] = int((o == -1).sum()), int((o == 0).sum()), int((o >= 1).sum())
        sl = slice(v * nr, (v + 1) * nr)
        g["rays_hit"] = int((hits["voxel"][sl] != qr.INVALID).sum())
        g["rays_in_map"] = int((hits["cells"][sl] > 0).sum())
        g["ray_cells"] = int(hits["cells"][sl].astype(np.int64).sum())
        g["ray_unknown"] = int(unk[v].astype(np.int64).sum())
    return gain, {k: x.reshape(nv, nr) for k, x in hits.items()}, unk


def unambiguous_rays(geo, views, n, seed):
    """n ray vectors (float32, not normalised, all directions) none of which is ambiguous (query_ref.segment_ambiguous) for
    ANY of the views: 4 n candidates are drawn, the first n that every view clears are kept; fewer than n is an error.
    Views with a non-finite number are left out of the test: their rays visit nothing, whatever the vector."""
    cand = np.random.default_rng(seed).normal(0.0, 1.0, (4 * n, 3)).astype(F)
    a, b, given = rays_of(views, cand)
    keep = np.ones(len(cand), bool)
    for v in range(len(a)):
        if given[v].all():
            keep &= ~qr.segment_ambiguous(geo, a[v], b[v])
    if keep.sum() < n:
        raise ValueError("only %d of %d candidate rays are unambiguous for every view; %d wanted" % (keep.sum(), len(cand), n))
    return np.ascontiguousarray(cand[keep][:n])


def equal_gain(got, ref):
    """None if every field of every VIEW_GAIN entry is equal, else a message"""
    for k in binding.VIEW_GAIN.names:
        bad = np.flatnonzero(got[k] != ref[k])
        if len(bad):
            return "%s differs at views %s: got %s, expected %s" % (k, bad[:5], got[k][bad[:5]], ref[k][bad[:5]])
    return None


def standard_views(geo, seed):
    """the eight views the tests put on a map: four inside it (two of them among the first min(N, 32) cells of every
    axis, where the crafted random blocks have their obstacles) with random orientations, one outside looking in along
    +x, one with range 0, one with NaN in pos, one whose range exceeds the map's diagonal.  Positions lie in the middle
    half of their cells (a zero-length ray is then never near a plane)."""
    rng = np.random.default_rng(seed)
    size = F(1) / geo.recip
    origin = geo.center + geo.pmin
    longest = float(geo.N.max()) * float(size)

    def inside(limit):
        u = rng.integers(0, limit) + rng.uniform(0.25, 0.75, 3)
        return (origin + u.astype(F) * size).astype(F)

    def quat():
        q = rng.normal(0.0, 1.0, 4)
        return (q / np.linalg.norm(q)).astype(F)

    v = np.zeros(8, binding.VIEW)
    sub = np.minimum(geo.N, 32)
    for i, limit in enumerate((sub, sub, geo.N, geo.N, None, geo.N, geo.N, sub)):
        if limit is not None:
            v[i]["pos"], v[i]["q"], v[i]["range"] = inside(limit), quat(), 0.3 * longest
    u_out = np.array([-2.4, 0.45 * geo.N[1] + 0.3, 0.55 * geo.N[2] + 0.3])
    v[4]["pos"], v[4]["range"] = (origin + u_out.astype(F) * size).astype(F), 0.75 * longest
    v[4]["q"] = (np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0)     # the camera's z axis along +x
    v[5]["range"] = 0.0
    v[6]["pos"][1] = np.nan
    v[7]["range"] = 2.5 * float(np.linalg.norm(geo.N)) * float(size)
    return v
