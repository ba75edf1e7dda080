"""The world mesh (include/sdm.h: sdm_world_mesh_update / sdm_get_world_mesh_info / sdm_get_world_mesh_faces /
sdm_get_world_mesh_vertices) restated for the tests, twice: build_cells, a plain loop per cell and direction over a dict
of world cells, and BrickModel, vectorised over the bricks.  Both take the archive as world_bricks() returns it (WORLD_BRICK
headers in brick order, 512 words each) and the keywords of SdmMap.world_mesh_update.  Everything is integer except xyz:
one float32 multiplication a coordinate."""
import numpy as np

from semantic_dsp_map_amd import binding

# direction -> (axis, step): the outward normal; [dir][q] -> the corner's offset from the cell: sdm.h's table ("surface mesh")
DIRS = [(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]
QUAD = np.array([
    [[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0]],
    [[1, 0, 0], [1, 1, 0], [1, 1, 1], [1, 0, 1]],
    [[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]],
    [[0, 1, 0], [0, 1, 1], [1, 1, 1], [1, 1, 0]],
    [[0, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0]],
    [[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]],
], np.int64)
KEYS = ("labels", "track", "static_only", "movable_only", "observed_only", "skip_unknown_faces", "skip_absent_faces", "box", "max_faces",
        "max_vertices")


def options(**kw):
    assert set(kw) <= set(KEYS), kw
    o = dict(labels=None, track=-1, static_only=False, movable_only=False, observed_only=False, skip_unknown_faces=False,
             skip_absent_faces=False, box=None, max_faces=0, max_vertices=0)
    o.update(kw)
    return o


def flags_of(o):
    return ((binding.WORLD_MESH_STATIC_ONLY if o["static_only"] else 0) | (binding.WORLD_MESH_MOVABLE_ONLY if o["movable_only"] else 0) |
            (binding.WORLD_MESH_OBSERVED_ONLY if o["observed_only"] else 0) | (binding.WORLD_MESH_SKIP_UNKNOWN_FACES if o["skip_unknown_faces"] else 0) |
            (binding.WORLD_MESH_SKIP_ABSENT_FACES if o["skip_absent_faces"] else 0) | (binding.WORLD_MESH_BOX if o["box"] is not None else 0))


def solid_of(words, max_movable, o):
    """the options' rule on an array of archived words"""
    w = np.asarray(words, np.uint32)
    occ = ((w >> 24) & 0xFF).astype(np.uint8).view(np.int8).astype(np.int32)
    label, track = ((w >> 16) & 0xFF).astype(np.int64), (w & 0xFFFF).astype(np.int64)
    solid = (occ == 1) if o["observed_only"] else (occ >= 1)
    allowed = np.ones(256, bool)
    if o["labels"] is not None:
        allowed[:] = False
        allowed[[int(l) for l in o["labels"]]] = True
    solid = solid & allowed[label]
    if o["track"] != -1:
        solid = solid & (track == o["track"])
    movable = (track >= 1) & (track <= max_movable)
    if o["static_only"]:
        solid = solid & ~movable
    if o["movable_only"]:
        solid = solid & movable
    return solid


def in_box(coord, o):
    if o["box"] is None:
        return np.ones(len(coord), bool)
    lo, hi = np.asarray(o["box"][0], np.int64), np.asarray(o["box"][1], np.int64)
    return ((coord >= lo) & (coord <= hi)).all(axis=1)


def coords_of(hdr):
    return np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int64).reshape(-1, 3)


def finish(coord, rank, cell, d, kind, word, n_solid, o, stamp, voxel_size):
    """the lists and the info from the faces in order: per face its brick rank, world cell, dir, kind and the cell's word"""
    n = len(d)
    faces = np.zeros(n, binding.WORLD_MESH_FACE)
    cell = np.asarray(cell, np.int64).reshape(-1, 3)
    d, word = np.asarray(d, np.int64), np.asarray(word, np.uint32)
    local = cell & 7
    faces["brick"], faces["cell"] = rank, local[:, 0] | (local[:, 1] << 3) | (local[:, 2] << 6)
    faces["dir"], faces["kind"] = d, kind
    faces["track"], faces["label"], faces["occ"] = word & 0xFFFF, (word >> 16) & 0xFF, ((word >> 24) & 0xFF).astype(np.uint8).view(np.int8)
    corner = (cell[:, None, :] + QUAD[d]).reshape(-1, 3) if n else np.zeros((0, 3), np.int64)
    # a corner's place in the vertex order as one number: (owner bz, by, bx, local word), 17 bits an owner coordinate
    own, loc = (corner >> 3) + 32768, corner & 7
    key = (own[:, 2] << 43) | (own[:, 1] << 26) | (own[:, 0] << 9) | (loc[:, 2] << 6) | (loc[:, 1] << 3) | loc[:, 0]
    ukey, first = np.unique(key, return_index=True)
    used = corner[first]
    quads = np.searchsorted(ukey, key).astype(np.uint32).reshape(-1, 4)
    corners = used.astype(np.int32)
    xyz = (corners.astype(np.float32) * np.float32(voxel_size)).astype(np.float32)
    info = np.zeros(1, binding.WORLD_MESH_INFO)
    info["n_bricks"], info["n_vertex_bricks"] = len(coord), len(np.unique(used >> 3, axis=0)) if len(used) else 0
    info["n_faces"], info["n_vertices"], info["n_solid"], info["stamp"] = n, len(used), n_solid, stamp
    info["faces_by_dir"][0], info["faces_by_kind"][0] = np.bincount(d, minlength=6), np.bincount(np.asarray(kind, np.int64), minlength=4)
    io = info["options"]
    io["flags"], io["track"], io["max_faces"], io["max_vertices"] = flags_of(o), o["track"], o["max_faces"], o["max_vertices"]
    io["labels"][0] = np.full(8, 0xFFFFFFFF, np.uint32) if o["labels"] is None else binding.label_mask(o["labels"])
    if o["box"] is not None:
        io["bmin"][0], io["bmax"][0] = o["box"][0], o["box"][1]
    over = (o["max_faces"] > 0 and n > o["max_faces"]) or (o["max_vertices"] > 0 and len(used) > o["max_vertices"])
    return dict(coords=coord.astype(np.int16).reshape(-1, 3), faces=faces, quads=quads, corners=corners.reshape(-1, 3), xyz=xyz.reshape(-1, 3),
                info=info[0], over=bool(over))


def build_cells(hdr, cells, max_movable, stamp=0, voxel_size=0.1, **kw):
    """the contract, cell by cell"""
    o = options(**kw)
    coord = coords_of(hdr)
    cells = np.asarray(cells, np.uint32).reshape(-1, 512)
    world = {}
    for b, w in zip(coord.tolist(), cells):
        for c in range(512):
            world[(b[0] * 8 + (c & 7), b[1] * 8 + ((c >> 3) & 7), b[2] * 8 + (c >> 6))] = int(w[c])
    distinct = np.unique(cells)
    is_solid = dict(zip(distinct.tolist(), solid_of(distinct, max_movable, o).tolist()))
    solid = is_solid.__getitem__
    field = coord[in_box(coord, o)]
    rank, cell, d, kind, word, n_solid = [], [], [], [], [], 0
    for r, b in enumerate(field.tolist()):
        for c in range(512):
            g = (b[0] * 8 + (c & 7), b[1] * 8 + ((c >> 3) & 7), b[2] * 8 + (c >> 6))
            if not solid(world[g]):
                continue
            n_solid += 1
            for k, (axis, step) in enumerate(DIRS):
                q = list(g)
                q[axis] += step
                nw = world.get(tuple(q)) if all(-32768 <= (v >> 3) <= 32767 for v in q) else None
                if nw is None:
                    kd = 2
                elif solid(nw):
                    continue
                else:
                    nocc = ((nw >> 24) & 0xFF) - (256 if (nw >> 24) & 0x80 else 0)
                    kd = 1 if nocc == -1 else 0 if nocc == 0 else 3
                if (kd == 1 and o["skip_unknown_faces"]) or (kd == 2 and o["skip_absent_faces"]):
                    continue
                rank.append(r), cell.append(g), d.append(k), kind.append(kd), word.append(world[g])
    return finish(field, rank, cell, d, kind, word, n_solid, o, stamp, voxel_size)


class BrickModel:
    """the same, vectorised over the bricks: every brick's words in a 10 x 10 x 10 block with the facing slabs of its six
    neighbour bricks round them, ABSENT where the archive has no brick"""
    ABSENT = np.int64(-1)

    def __init__(self, hdr, cells, max_movable, stamp=0, voxel_size=0.1, **kw):
        o = options(**kw)
        coord = coords_of(hdr)
        n = len(coord)
        words = np.asarray(cells, np.uint32).reshape(n, 8, 8, 8).astype(np.int64)          # [brick, cz, cy, cx]
        pad = np.full((n, 10, 10, 10), self.ABSENT, np.int64)
        pad[:, 1:9, 1:9, 1:9] = words
        at = {tuple(b): i for i, b in enumerate(coord.tolist())}
        sl = slice(1, 9)
        for i, b in enumerate(coord.tolist()):
            for axis, step in DIRS:
                q = list(b)
                q[axis] += step
                j = at.get(tuple(q)) if -32768 <= q[axis] <= 32767 else None
                if j is None:
                    continue
                dst, src = [sl, sl, sl], [slice(None)] * 3
                dst[2 - axis], src[2 - axis] = (9 if step > 0 else 0), (0 if step > 0 else 7)
                pad[(i,) + tuple(dst)] = words[(j,) + tuple(src)]
        absent = pad == self.ABSENT
        solid = solid_of(np.where(absent, 0xFF000000, pad).astype(np.uint32), max_movable, o) & ~absent
        occ = ((np.where(absent, 0, pad) >> 24) & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64)
        field = np.flatnonzero(in_box(coord, o))
        own = solid[field][:, 1:9, 1:9, 1:9]
        has = np.zeros((len(field), 8, 8, 8, 6), bool)
        kinds = np.zeros((len(field), 8, 8, 8, 6), np.uint8)
        for k, (axis, step) in enumerate(DIRS):
            win = [sl, sl, sl]
            win[2 - axis] = slice(1 + step, 9 + step)
            win = (field,) + tuple(win)
            kd = np.where(absent[win], 2, np.where(occ[win] == -1, 1, np.where(occ[win] == 0, 0, 3))).astype(np.uint8)
            face = own & ~solid[win]
            if o["skip_unknown_faces"]:
                face &= kd != 1
            if o["skip_absent_faces"]:
                face &= kd != 2
            has[..., k], kinds[..., k] = face, kd
        r, z, y, x, d = np.nonzero(has)            # C order: ascending (brick rank, cell word, dir)
        fc = coord[field]
        cell = fc[r] * 8 + np.stack([x, y, z], 1) if len(r) else np.zeros((0, 3), np.int64)
        out = finish(fc, r, cell, d, kinds[r, z, y, x, d], words[field][r, z, y, x].astype(np.uint32), int(own.sum()), o, stamp, voxel_size)
        self.__dict__.update(out)
        self.opt = o


def answer(ref):
    r = ref if isinstance(ref, dict) else ref.__dict__
    return {k: r[k] for k in ("coords", "faces", "quads", "corners", "xyz", "info")}


def difference(got, want):
    """None if the two answers are the same bytes, else the first array that differs"""
    for k in ("coords", "faces", "quads", "corners", "xyz", "info"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            return "%s differs: %r / %r" % (k, a if a.size < 40 else a.shape, b if b.size < 40 else b.shape)
    return None
