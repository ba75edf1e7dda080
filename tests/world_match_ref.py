"""NumPy restatement of the world match (include/sdm.h: sdm_world_match), on top of tests/world_ref.py and
tests/world_io_ref.py, for the tests.

Written twice, as world_ref.py is.  dense() is the grid model: the sources that stay (the lowest index of each
coordinate) and the archive's bricks are rendered as a class grid and a label grid - the sources over their bounding box,
the archive over that box moved by the centre and grown by the radius - and the source grid is slid over the archive grid,
one slice per candidate.  naive() goes cell by cell over world_ref.Naive's dict from world cell to word and knows nothing of
bricks or grids; it also picks best and runner-up with loops of its own.  tests/test_world_match_ref.py holds the first
against the second.

Both take the archive as (headers, cells) the way world_bricks() returns them, and return (result, scores) in the binding's
dtypes, so a test compares bytes."""
import numpy as np

from semantic_dsp_map_amd import binding
from tests import world_io_ref as io
from tests import world_ref as wr

INT64_MIN = -(1 << 63)
UNK, FREE, OCC = 0, 1, 2


def classes(words, max_movable, flags):
    """0 unknown, 1 free, 2 occupied: a cell counts iff it would write under the flags"""
    w = np.asarray(words, np.uint32)
    return np.where(wr.writes(w, max_movable, flags), np.where(wr.occ_of(w) >= 1, OCC, FREE), UNK).astype(np.uint8)


def labels(words):
    return ((np.asarray(words, np.uint32) >> 16) & 0xFF).astype(np.uint8)


def candidates(offset, radius):
    """(d [n, 3] int64 in candidate order - x fastest -, the offsets centre + d)"""
    r = [int(v) for v in radius]
    dz, dy, dx = np.meshgrid(np.arange(-r[2], r[2] + 1), np.arange(-r[1], r[1] + 1), np.arange(-r[0], r[0] + 1), indexing="ij")
    d = np.stack([dx.ravel(), dy.ravel(), dz.ravel()], 1).astype(np.int64)
    return d, d + np.asarray(offset, np.int64)


def score_of(sc, weights):
    w = [int(v) for v in weights]
    return (w[0] * sc["n_oo"].astype(np.int64) + w[1] * sc["n_same"].astype(np.int64) + w[2] * sc["n_of"].astype(np.int64) +
            w[3] * sc["n_fo"].astype(np.int64) + w[4] * sc["n_ff"].astype(np.int64))


def render(hdr, cells, lo, size, max_movable, flags):
    """the bricks as (class, label) grids [z, y, x] over the box of world cells lo .. lo + size - 1"""
    cls, lab = np.zeros(tuple(int(v) for v in size[::-1]), np.uint8), np.zeros(tuple(int(v) for v in size[::-1]), np.uint8)
    cells = np.asarray(cells, np.uint32).reshape(-1, 512)
    for i, key in enumerate(io.coords(hdr)):
        at = np.array(key, np.int64) * 8 - lo                       # the brick's first cell inside the box
        a, b = np.maximum(at, 0), np.minimum(at + 8, size)
        if (a >= b).any():
            continue
        brick = cells[i].reshape(8, 8, 8)                            # [cz, cy, cx]
        src = tuple(slice(int(a[k] - at[k]), int(b[k] - at[k])) for k in (2, 1, 0))
        dst = tuple(slice(int(a[k]), int(b[k])) for k in (2, 1, 0))
        cls[dst], lab[dst] = classes(brick[src], max_movable, flags), labels(brick[src])
    return cls, lab


def dense(hdr, cells, arch_hdr, arch_cells, offset=(0, 0, 0), radius=(2, 2, 1), weights=binding.WORLD_MATCH_WEIGHTS, max_movable=0, flags=0):
    """one sdm_world_match on the grid model; flags: STATIC_ONLY | OBSERVED_ONLY"""
    hdr, cells = np.asarray(hdr), np.asarray(cells, np.uint32).reshape(-1, 512)
    c, r = np.asarray(offset, np.int64), np.asarray(radius, np.int64)
    assert (np.abs(c) <= io.MAX_OFFSET).all() and ((r >= 0) & (r <= binding.WORLD_MATCH_MAX_RADIUS)).all()
    d, off = candidates(c, r)
    sc = np.zeros(len(d), binding.WORLD_MATCH_SCORE)
    sc["offset"] = off
    res = np.zeros(1, binding.WORLD_MATCH_RESULT)[0]
    res["n_candidates"] = len(d)
    first = sorted(io.first_of_each(hdr).values())
    if first:
        b = np.array(io.coords(hdr[first]), np.int64)
        lo, size = b.min(axis=0) * 8, (b.max(axis=0) - b.min(axis=0) + 1) * 8
        assert int(np.prod(size + 2 * r)) < 1 << 27, "the sources lie too far apart for the grid model"
        s_cls, s_lab = render(hdr[first], cells[first], lo, size, max_movable, flags)
        a_cls, a_lab = render(arch_hdr, arch_cells, lo + c - r, size + 2 * r, max_movable, flags)
        res["n_sources"], res["src_occupied"], res["src_free"] = len(first), (s_cls == OCC).sum(), (s_cls == FREE).sum()
        s_occ, s_free = s_cls == OCC, s_cls == FREE
        for k, dk in enumerate(d + r):                               # the archive grid's slice under this candidate
            win = tuple(slice(int(dk[a]), int(dk[a] + size[a])) for a in (2, 1, 0))
            w_cls, w_lab = a_cls[win], a_lab[win]
            oo = s_occ & (w_cls == OCC)
            sc[k]["n_oo"], sc[k]["n_of"] = oo.sum(), (s_occ & (w_cls == FREE)).sum()
            sc[k]["n_fo"], sc[k]["n_ff"] = (s_free & (w_cls == OCC)).sum(), (s_free & (w_cls == FREE)).sum()
            sc[k]["n_same"] = (oo & (s_lab == w_lab)).sum()
    s = score_of(sc, weights)
    best = int(np.lexsort((np.arange(len(d)), (d * d).sum(axis=1), -s))[0])
    far = np.abs(d - d[best]).max(axis=1) >= 2
    res["best"], res["best_offset"], res["best_score"] = best, off[best], s[best]
    res["runner_up"] = s[far].max() if far.any() else INT64_MIN
    return res, sc


def naive_archive(arch_hdr, arch_cells):
    """world_ref.Naive holding every word of the bricks that is not the unknown word"""
    A = wr.Naive()
    arch_cells = np.asarray(arch_cells, np.uint32).reshape(-1, 512)
    for i, key in enumerate(io.coords(arch_hdr)):
        for w in np.nonzero(arch_cells[i] != wr.UNKNOWN)[0].tolist():
            A.cell[tuple(8 * key[a] + ((w >> (3 * a)) & 7) for a in range(3))] = int(arch_cells[i][w])
    return A


def naive(hdr, cells, A, offset=(0, 0, 0), radius=(2, 2, 1), weights=binding.WORLD_MATCH_WEIGHTS, max_movable=0, flags=0):
    """one sdm_world_match cell by cell; A: a world_ref.Naive"""
    cells = np.asarray(cells, np.uint32).reshape(-1, 512)
    c, r, w = [int(v) for v in offset], [int(v) for v in radius], [int(v) for v in weights]

    known = {}

    def cls(word):
        if word not in known:                                        # (few distinct words: one evaluation of the rule each)
            known[word] = int(classes(np.uint32(word), max_movable, flags))
        return known[word]

    seen, src = set(), []                                            # (world cell, class, label) of every counted source cell
    for i, key in enumerate(io.coords(hdr)):
        if key in seen:
            continue
        seen.add(key)
        for cw in range(512):
            k = cls(cells[i][cw])
            if k != UNK:
                src.append((tuple(8 * key[a] + ((cw >> (3 * a)) & 7) for a in range(3)), k, (int(cells[i][cw]) >> 16) & 0xFF))
    rows = []
    for dz in range(-r[2], r[2] + 1):
        for dy in range(-r[1], r[1] + 1):
            for dx in range(-r[0], r[0] + 1):
                d = (dx, dy, dz)
                n = dict(oo=0, of=0, fo=0, ff=0, same=0)
                for g, k, lab in src:
                    at = tuple(g[a] + c[a] + d[a] for a in range(3))
                    if not io.in_range([v >> 3 for v in at]):
                        continue
                    word = A.word(at)
                    ka = cls(word)
                    if ka == UNK:
                        continue
                    n["fo"[k - 1] + "fo"[ka - 1]] += 1
                    if k == OCC and ka == OCC and ((word >> 16) & 0xFF) == lab:
                        n["same"] += 1
                score = w[0] * n["oo"] + w[1] * n["same"] + w[2] * n["of"] + w[3] * n["fo"] + w[4] * n["ff"]
                rows.append((d, n, score))
    best = 0
    for k, (d, n, score) in enumerate(rows):
        bd, _, bs = rows[best]
        if score > bs or (score == bs and sum(v * v for v in d) < sum(v * v for v in bd)):
            best = k
    runner = [score for d, n, score in rows if max(abs(d[a] - rows[best][0][a]) for a in range(3)) >= 2]
    sc = np.zeros(len(rows), binding.WORLD_MATCH_SCORE)
    for k, (d, n, score) in enumerate(rows):
        sc[k]["offset"] = [c[a] + d[a] for a in range(3)]
        sc[k]["n_oo"], sc[k]["n_of"], sc[k]["n_fo"], sc[k]["n_ff"], sc[k]["n_same"] = n["oo"], n["of"], n["fo"], n["ff"], n["same"]
    res = np.zeros(1, binding.WORLD_MATCH_RESULT)[0]
    res["n_candidates"], res["n_sources"] = len(rows), len(seen)
    res["src_occupied"], res["src_free"] = sum(k == OCC for _, k, _ in src), sum(k == FREE for _, k, _ in src)
    res["best"], res["best_offset"], res["best_score"] = best, sc[best]["offset"], rows[best][2]
    res["runner_up"] = max(runner) if runner else INT64_MIN
    return res, sc


# ---- the planted-offset scene: a non-periodic archive of random blobs, and a copy of it that believes in another origin
PLANTED = (3, -2, 1)


def blob_scene(seed=3, n_blobs=9, extent=40):
    """(headers, cells) of an archive of random ellipsoid blobs: their shells occupied, labelled by blob, the cells round them
    free - a few hundred occupied cells that repeat under no shift"""
    rng = np.random.default_rng(seed)
    grid = np.full((extent, extent, extent), wr.UNKNOWN, np.uint32)
    z, y, x = np.meshgrid(*(np.arange(extent),) * 3, indexing="ij")
    for b in range(n_blobs):
        centre, axes = rng.uniform(7, extent - 7, 3), rng.uniform(1.6, 4.5, 3)
        q = ((x - centre[0]) / axes[0]) ** 2 + ((y - centre[1]) / axes[1]) ** 2 + ((z - centre[2]) / axes[2]) ** 2
        grid[(q > 1.0) & (q <= 2.6) & (grid == wr.UNKNOWN)] = 0                              # free air round it
        grid[(q > 0.45) & (q <= 1.0)] = np.uint32(1 << 24 | (b + 1) << 16 | (1000 + b))      # the shell
    nb = extent // 8
    cells = grid.reshape(nb, 8, nb, 8, nb, 8).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 512)
    bz, by, bx = np.meshgrid(*(np.arange(nb),) * 3, indexing="ij")
    coord = np.stack([bx.ravel(), by.ravel(), bz.ravel()], 1) - 2                            # astride 0
    keep = (cells != wr.UNKNOWN).any(axis=1)
    return io.make_headers(coord[keep], 1, 2), np.ascontiguousarray(cells[keep])


def shifted_copy(hdr, cells, shift):
    """the same cells as bricks of a frame whose origin lies `shift` cells further: world cell g becomes g - shift, so
    importing the copy under cell_offset == shift puts every cell back"""
    A = io.Archive(1 << 20)
    io.import_bricks(A, hdr, cells, tuple(-int(v) for v in shift), 0, 0)
    return A.bricks()
