"""NumPy restatement of the ground layer (include/sdm.h: sdm_ground_update / sdm_get_ground / sdm_query_ground /
sdm_query_footprints), for the tests.

Input is the snapshot grid esdf_ref.snapshot_grid gives - the second result word (track | label << 16 | occ << 24) of every
cell, indexed [z, y, x] in map-index order - and the options as a dict (up, h_lo, h_hi, clearance, max_step, labels,
flags).  Everything is integer except the few float32 operations of the two queries, restated one operation at a time.
"""
import numpy as np

from semantic_dsp_map_amd import binding
from tests import esdf_ref as er

UNKNOWN_PASSABLE, IGNORE_MOVABLE, NONE_IS_LETHAL = 0x1, 0x2, 0x4
NO_LEVEL = 0xFFFF
INVALID = 0xFFFFFFFF
INT32_MIN = -(1 << 31)


def options(up, h_lo, h_hi, clearance=0, max_step=0, labels=(), flags=0):
    return dict(up=(int(up[0]), int(up[1])), h_lo=int(h_lo), h_hi=int(h_hi), clearance=int(clearance), max_step=int(max_step),
                labels=sorted(int(l) for l in labels), flags=int(flags))


def update_kwargs(opt):
    """the options as SdmMap.ground_update takes them"""
    return dict(up=opt["up"], h_lo=opt["h_lo"], h_hi=opt["h_hi"], clearance=opt["clearance"], max_step=opt["max_step"],
                support_labels=opt["labels"], unknown_passable=bool(opt["flags"] & UNKNOWN_PASSABLE),
                ignore_movable=bool(opt["flags"] & IGNORE_MOVABLE), none_is_lethal=bool(opt["flags"] & NONE_IS_LETHAL))


def grid_axes(up_axis):
    """(u, v): the other two map axes, ascending"""
    return tuple(a for a in (0, 1, 2) if a != up_axis)


def columns(grid, up):
    """a [z, y, x] grid -> [j_v, i_u, h]: the grid's columns in height order"""
    axis, sign = up
    au, av = grid_axes(axis)
    g = np.transpose(grid, (2 - av, 2 - au, 2 - axis))
    return g[:, :, ::-1] if sign < 0 else g


def cell_classes(w1, max_movable, opt):
    """-> (solid, passable, candidate, unknown, label) of the result words w1 (any shape)"""
    w = np.asarray(w1, np.uint32)
    occ = ((w >> 24) & 0xFF).astype(np.uint8).view(np.int8).astype(np.int32)
    track = (w & 0xFFFF).astype(np.int32)
    label = ((w >> 16) & 0xFF).astype(np.int32)
    movable = (track >= 1) & (track <= max_movable)
    solid = occ >= 1
    passable = occ == 0
    if opt["flags"] & IGNORE_MOVABLE:
        passable = passable | (solid & movable)
        solid = solid & ~movable
    if opt["flags"] & UNKNOWN_PASSABLE:
        passable = passable | (occ == -1)
    allowed = np.zeros(256, bool)
    allowed[list(opt["labels"])] = True
    return solid, passable, solid & ~movable & allowed[label], occ == -1, label


def _highest(mask):
    """per column the highest h with mask[..., h], -1 if none"""
    N = mask.shape[-1]
    at = N - 1 - np.argmax(mask[..., ::-1], axis=-1)
    return np.where(mask.any(axis=-1), at, -1)


def build(snap, max_movable, opt):
    """-> (cells GROUND_CELL [N_v, N_u], d2 uint32 [N_v, N_u], info dict)"""
    col = columns(snap, opt["up"])
    NV, NU, N = col.shape
    solid, passable, cand, unknown, label = cell_classes(col, max_movable, opt)
    # run[h]: the consecutive passable cells directly above h, up to the map's top; above the top everything is passable
    run = np.zeros(col.shape, np.int64)
    for h in range(N - 2, -1, -1):
        run[..., h] = np.where(passable[..., h + 1], run[..., h + 1] + 1, 0)
    h_all = np.arange(N)
    band = (h_all >= opt["h_lo"]) & (h_all <= opt["h_hi"])
    open_top = run == (N - 1 - h_all)
    support = cand & band & (open_top | (run >= opt["clearance"]))
    level, top = _highest(support), _highest(solid & band)
    has = level >= 0
    jj, ii = np.meshgrid(np.arange(NV), np.arange(NU), indexing="ij")
    at = np.maximum(level, 0)
    cells = np.zeros((NV, NU), binding.GROUND_CELL)
    cells["level"] = np.where(has, level, NO_LEVEL)
    cells["top"] = np.where(top >= 0, top, NO_LEVEL)
    cells["label"] = np.where(has, label[jj, ii, at], 0)
    cells["headroom"] = np.where(has, np.minimum(run[jj, ii, at], 255), 0)
    cells["n_unknown"] = np.minimum((unknown & band).sum(axis=-1), 255)
    klass = np.where(has, 1, np.where(top >= 0, 2, 0))
    # step: a 4-neighbour inside the grid with a level that lies more than max_step below
    step = np.zeros((NV, NU), bool)
    lv = level.astype(np.int64)
    for dj, di in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        nb = np.full((NV, NU), -1, np.int64)
        src = lv[max(dj, 0):NV + min(dj, 0), max(di, 0):NU + min(di, 0)]
        nb[max(-dj, 0):NV - max(dj, 0), max(-di, 0):NU - max(di, 0)] = src
        step |= has & (nb >= 0) & (lv > nb + opt["max_step"])
    lethal = (klass == 2) | step
    if opt["flags"] & NONE_IS_LETHAL:
        lethal |= klass == 0
    cells["cls"] = klass | (step.astype(np.int64) << 2) | (lethal.astype(np.int64) << 3)
    d2 = er.edt_d2(lethal[None])[0]
    au, av = grid_axes(opt["up"][0])
    info = dict(n_u=NU, n_v=NV, axis_u=au, axis_v=av, n_ground=int((klass == 1).sum()), n_obstacle=int((klass == 2).sum()),
                n_none=int((klass == 0).sum()), n_step=int(step.sum()), n_lethal=int(lethal.sum()),
                level_min=int(level[has].min()) if has.any() else NO_LEVEL, level_max=int(level[has].max()) if has.any() else NO_LEVEL)
    return cells, d2, info


def check_info(info, ref, opt):
    """a GROUND_INFO record against build()'s dict and the options (None, or a message)"""
    for k, v in ref.items():
        if int(info[k]) != v:
            return "%s: %d, expected %d" % (k, int(info[k]), v)
    o = info["options"]
    got = (int(o["up_axis"]), int(o["up_sign"]), int(o["h_lo"]), int(o["h_hi"]), int(o["clearance"]), int(o["max_step"]), int(o["flags"]))
    want = (opt["up"][0], opt["up"][1], opt["h_lo"], opt["h_hi"], opt["clearance"], opt["max_step"], opt["flags"])
    if got != want or not np.array_equal(o["support_labels"], binding.label_mask(opt["labels"])):
        return "options echoed as %r, expected %r" % (got, want)
    return None


def origin_of(geo):
    """the global position of the min corner of cell (0, 0, 0), float32 (layer_origin)"""
    return (geo.center + geo.pmin).astype(np.float32)


def query_ground(geo, voxel_size, opt, cells, d2, xyz):
    """-> GROUND_RESULT array as the kernel must return it"""
    size = np.float32(voxel_size)
    axis, sign = opt["up"]
    au, av = grid_axes(axis)
    u = geo.u(xyz)
    n = len(u)
    with np.errstate(invalid="ignore"):
        ok = ((u >= 0) & (u < geo.N.astype(np.float32))).all(axis=1)
    cell = np.floor(np.where(ok[:, None], u, 0)).astype(np.int64)
    out = np.zeros(n, binding.GROUND_RESULT)
    out["col"], out["d2"], out["above"], out["dist"], out["status"] = INVALID, INVALID, INT32_MIN, -1.0, 3
    out["cell"]["level"], out["cell"]["top"] = NO_LEVEL, NO_LEVEL
    i, j = cell[ok, au], cell[ok, av]
    NU, NA = int(geo.N[au]), int(geo.N[axis])
    r = out[ok]
    r["col"] = i + j * NU
    r["cell"] = cells[j, i]
    r["d2"] = d2[j, i]
    r["status"] = 0
    known = r["d2"] != INVALID
    dist = (np.sqrt(np.where(known, r["d2"], 0).astype(np.float32)) * size).astype(np.float32)
    r["dist"] = np.where(known, dist, np.float32(-1))
    level = r["cell"]["level"].astype(np.int64)
    has = level != NO_LEVEL
    h = cell[ok, axis] if sign > 0 else NA - 1 - cell[ok, axis]
    r["above"] = np.where(has, h - level, INT32_MIN)
    k = level + 1 if sign > 0 else NA - 1 - level
    surface = (origin_of(geo)[axis] + (k.astype(np.float32) * size).astype(np.float32)).astype(np.float32)
    r["surface"] = np.where(has, surface, np.float32(0))
    out[ok] = r
    return out


def covered(geo, voxel_size, up_axis, fp):
    """the footprint rule on every column of the grid -> bool [N_v, N_u] (float32, one operation at a time)"""
    size, half = np.float32(voxel_size), np.float32(0.5)
    au, av = grid_axes(up_axis)
    o = origin_of(geo)
    f = {k: np.float32(fp[k]) for k in binding.FOOTPRINT.names}
    pu = (o[au] + ((np.arange(geo.N[au]).astype(np.float32) + half) * size).astype(np.float32)).astype(np.float32)[None, :]
    pv = (o[av] + ((np.arange(geo.N[av]).astype(np.float32) + half) * size).astype(np.float32)).astype(np.float32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        du, dv = (pu - f["center_u"]).astype(np.float32), (pv - f["center_v"]).astype(np.float32)
        along = ((du * f["dir_u"]).astype(np.float32) + (dv * f["dir_v"]).astype(np.float32)).astype(np.float32)
        across = ((dv * f["dir_u"]).astype(np.float32) - (du * f["dir_v"]).astype(np.float32)).astype(np.float32)
        return (np.abs(along) <= f["half_len"]) & (np.abs(across) <= f["half_wid"])


def query_footprints(geo, voxel_size, opt, cells, d2, fps):
    """-> FOOTPRINT_RESULT array as the kernel must return it"""
    size = np.float32(voxel_size)
    fps = np.asarray(fps, binding.FOOTPRINT).reshape(-1)
    out = np.zeros(len(fps), binding.FOOTPRINT_RESULT)
    out["level_min"], out["level_max"], out["min_d2"], out["first_lethal"] = NO_LEVEL, NO_LEVEL, INVALID, INVALID
    NU = cells.shape[1]
    word = np.arange(cells.size, dtype=np.int64).reshape(cells.shape)
    klass, lethal = cells["cls"] & 3, (cells["cls"] & 8) != 0
    for k, fp in enumerate(fps):
        vals = np.array([fp[name] for name in binding.FOOTPRINT.names], np.float32)
        with np.errstate(over="ignore"):
            if not np.isfinite(vals).all() or np.float32(fp["half_len"] + fp["half_wid"]) > np.float32(64) * size:
                continue
        c = covered(geo, voxel_size, opt["up"][0], fp)
        if not c.any():
            continue
        r = out[k:k + 1]
        r["n_cols"], r["n_lethal"] = c.sum(), (c & lethal).sum()
        r["n_none"], r["n_ground"] = (c & (klass == 0)).sum(), (c & (klass == 1)).sum()
        g = c & (klass == 1)
        if g.any():
            r["level_min"], r["level_max"] = cells["level"][g].min(), cells["level"][g].max()
        r["min_d2"] = d2[c].min()
        if (c & lethal).any():
            r["first_lethal"] = word[c & lethal].min()
    assert NU == int(geo.N[grid_axes(opt["up"][0])[0]])
    return out
