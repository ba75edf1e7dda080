"""The crafted pairs of block and archive of the world changes tests, shared by tests/test_world_changes_ref.py (the two
restatements against each other, no GPU) and tests/test_world_changes_gpu.py (the library against them).  A case is a dict:
shape (a name of tests/shape_cases.py), steps (the ring's moved_steps), the block as occ / label / track grids [z, y, x]
(occ -1 never observed, 0 free, 1 occupied), the archive as hdr and cells for world_import, and builds - a list of (keywords
of the build, what is known about its answer in closed form: fields of the info record).  Plain numpy.

Block cells are named by their map index (x, y, z); world cell = g0 + index with g0 = steps - (N >> 1).  The archive is
written as a dense word grid over the candidates' box and cut into bricks (world_reach_cases.from_grid)."""
import itertools

import numpy as np

from semantic_dsp_map_amd import synth
from semantic_dsp_map_amd.binding import WORLD_CHANGE_APPEARED, WORLD_CHANGE_RELABELLED, WORLD_CHANGE_VANISHED
from tests import shape_cases as sc
from tests.world_reach_cases import FREE, UNKNOWN, from_grid

B, R, CAR = synth.LABEL_BUILDING, synth.LABEL_ROAD, synth.LABEL_CAR
TRACK = {B: synth.TRACK_BUILDING, R: synth.TRACK_ROAD, CAR: 3}     # CAR rides a movable track
FLAG_NAMES = ("face_connected", "by_label", "static_only", "observed_only")
FLAG_SETS = [dict(zip(FLAG_NAMES, v)) for v in itertools.product((False, True), repeat=4)]


def word(label, track=None, occ=1):
    return np.uint32((occ & 0xFF) << 24 | label << 16 | (TRACK[label] if track is None else track))


def dims(cfg):
    return np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.int64)


def steps_at(cfg, brick, off):
    """ring offsets that put the block's min corner at cell `off` of brick `brick`, per axis"""
    N = dims(cfg)
    return [int(8 * brick[a] + off[a] + (N[a] >> 1)) for a in range(3)]


def box_of(cfg, steps):
    """-> g0 (world cell of map index (0, 0, 0)), b0 (the first candidate brick), nb (candidates per axis)"""
    N = dims(cfg)
    g0 = np.asarray(steps, np.int64) - (N >> 1)
    b0 = g0 >> 3
    return g0, b0, ((g0 + N - 1) >> 3) - b0 + 1


class Pair:
    """a block and an archive grid over the block's candidates, written cell by cell in map indices"""

    def __init__(self, shape, steps, block_occ=0, archive=UNKNOWN):
        self.shape, self.cfg, self.steps = shape, sc.config(shape), [int(s) for s in steps]
        N = dims(self.cfg)
        self.g0, self.b0, self.nb = box_of(self.cfg, steps)
        self.occ = np.full(tuple(N[::-1]), block_occ, np.int8)
        self.label, self.track = np.zeros(self.occ.shape, np.uint8), np.zeros(self.occ.shape, np.uint16)
        self.grid = np.full(tuple(int(n) * 8 for n in self.nb[::-1]), UNKNOWN, np.uint32)
        o = self.g0 - self.b0 * 8
        self.inside = (slice(o[2], o[2] + N[2]), slice(o[1], o[1] + N[1]), slice(o[0], o[0] + N[0]))
        self.grid[self.inside] = archive
        self.skip, self.stamps = set(), {}

    def now(self, cell, label=None, occ=1, track=None):
        x, y, z = cell
        self.occ[z, y, x] = occ
        if label is not None:
            self.label[z, y, x], self.track[z, y, x] = label, TRACK[label] if track is None else track

    def before(self, cell, w):
        """the archived word at map index `cell` (which may lie outside the block, inside a candidate)"""
        at = self.g0 + np.asarray(cell, np.int64) - self.b0 * 8
        self.grid[at[2], at[1], at[0]] = w

    def case(self, builds):
        skip = set(self.skip) | {tuple(int(v) for v in self.b0 + np.array(k)) for k in itertools.product(*(range(int(n)) for n in self.nb))
                                 if not all(-32768 <= int(v) <= 32767 for v in self.b0 + np.array(k))}
        hdr, cells = from_grid(self.grid, tuple(int(v) for v in self.b0), skip)
        for j in range(len(hdr)):
            hdr["last_stamp"][j] = self.stamps.get((int(hdr["bx"][j]), int(hdr["by"][j]), int(hdr["bz"][j])), 1)
        return dict(shape=self.shape, steps=self.steps, occ=self.occ, label=self.label, track=self.track, hdr=hdr, cells=cells, builds=builds)


def block_words(c):
    """the block's word grid [z, y, x] as the restatements read it: what a map that holds the block would report"""
    w = (c["track"].astype(np.uint32) | (c["label"].astype(np.uint32) << 16) | (np.uint32(1) << 24))
    return np.where(c["occ"] == 1, w, np.where(c["occ"] == 0, np.uint32(FREE), np.uint32(UNKNOWN))).astype(np.uint32)


def every_flag_set(want=None, **kw):
    return [(dict(f, **kw), dict(want or {})) for f in FLAG_SETS]


# ---- every cell of the class table, on 4 x 4 x 4 cells: inside one brick (offset 0), astride two on y (1, 7, 1), on every axis (7)
def class_table(off=(1, 7, 1), builds=None):
    cfg = sc.config("A")
    p = Pair("A", steps_at(cfg, (3, -2, 4), off))
    p.now((0, 0, 0), B), p.before((0, 0, 0), FREE)                          # O / F
    p.now((1, 0, 0), occ=0), p.before((1, 0, 0), word(B))                   # F / O
    p.now((2, 0, 0), B), p.before((2, 0, 0), word(R))                       # O / O, another label
    p.now((3, 0, 0), B), p.before((3, 0, 0), word(B, track=5))              # O / O, the same label (another track)
    p.now((0, 1, 0), occ=0), p.before((0, 1, 0), FREE)                      # F / F
    p.now((1, 1, 0), R)                                                      # O / U
    p.now((2, 1, 0), occ=0)                                                  # F / U
    p.now((3, 1, 0), occ=-1), p.before((3, 1, 0), word(R))                  # U / O
    p.now((0, 2, 0), occ=-1), p.before((0, 2, 0), FREE)                     # U / F
    p.now((1, 2, 0), occ=-1)                                                 # U / U
    p.now((2, 2, 0), B), p.before((2, 2, 0), word(B, occ=2))                # the archive guessed: same, or new when only the observed count
    p.now((3, 2, 0), occ=0), p.before((3, 2, 0), word(CAR))                 # a movable track remembered: vanished, or new when only static
    p.now((0, 3, 0), CAR), p.before((0, 3, 0), FREE)                        # a movable track seen: appeared, or remembered
    p.before((5, 5, 5), word(B))                                             # candidates' cells outside the block: remembered
    if min(off[0], off[2]) >= 1 and off[1] >= 6:
        p.before((-1, -6, -1), FREE)
    return p.case(every_flag_set() if builds is None else builds)


# ---- regions of chosen shapes on 8 x 4 x 128 cells whose seams on all three axes run through the block
def _shapes():
    """name -> [(map index, label)]: seams between x = 3 | 4, y = 1 | 2 and z = 3 | 4, 11 | 12, ..., 35 | 36, ..."""
    serp = [(0, 0, z) for z in range(70, 101)] + [(x, 0, 100) for x in range(1, 8)] + [(7, 0, z) for z in range(70, 100)]
    return {
        "face": [((3, 0, 1), B), ((4, 0, 1), B)],
        "edge": [((3, 1, 20), B), ((4, 2, 20), B)],
        "corner": [((3, 1, 35), B), ((4, 2, 36), B)],          # they touch where eight bricks meet
        "bridge_class": [((2, 3, 50), B), ((4, 3, 50), B)],    # the cell between them has the other class
        "bridge_label": [((2, 0, 60), B), ((3, 0, 60), R), ((4, 0, 60), B)],
        "serpentine": [(c, R) for c in serp],
    }


SHAPE_STEPS = steps_at(sc.config("C"), (3, -2, 5), (4, 6, 4))
N_SHAPE_CELLS = sum(len(v) for v in _shapes().values()) + 1           # (the bridge's middle cell)


def shape_builds(cls_main, cls_mid):
    """26-connected: face, edge, corner, bridge_class's two ends and its middle, bridge_label, serpentine = 8 regions; by label
    bridge_label falls into 3; face-connected the edge and the corner pair fall apart"""
    out = []
    for face, by_label in itertools.product((False, True), repeat=2):
        total = 8 + (2 if by_label else 0) + (2 if face else 0)
        out.append((dict(face_connected=face, by_label=by_label), dict(n_regions_total=total, n_regions=total, n_cells=N_SHAPE_CELLS)))
    out.append((dict(min_cells=3), dict(n_regions_total=8, n_regions=2, n_cells=N_SHAPE_CELLS)))
    out.append((dict(min_cells=3, by_label=True), dict(n_regions_total=10, n_regions=1)))
    out.append((dict(classes=(cls_main,)), dict(n_regions_total=7, n_cells=N_SHAPE_CELLS - 1)))
    out.append((dict(classes=(cls_mid, WORLD_CHANGE_RELABELLED)), dict(n_regions_total=1, n_cells=1)))
    out.append((dict(labels=(R,)), dict(n_cells=len(_shapes()["serpentine"]) + 1)))
    out.append((dict(labels=()), dict(n_cells=0, n_bricks=0, n_regions_total=0)))
    out.append((dict(classes=()), dict(n_cells=0, n_bricks=0, n_regions_total=0)))
    return out


def vanished_shapes():
    """an all-free block over an archived pattern; one brick of the block is absent from the archive"""
    p = Pair("C", SHAPE_STEPS, block_occ=0, archive=FREE)
    for cells in _shapes().values():
        for c, label in cells:
            p.before(c, word(label))
    p.now((3, 3, 50), B), p.before((3, 3, 50), FREE)
    p.skip.add(tuple(int(v) for v in (p.g0 + np.array([6, 3, 110])) >> 3))
    return p.case(shape_builds(WORLD_CHANGE_VANISHED, WORLD_CHANGE_APPEARED))


def appeared_shapes():
    """the reverse: the block holds the pattern, the archive remembers free space"""
    p = Pair("C", SHAPE_STEPS, block_occ=0, archive=FREE)
    for cells in _shapes().values():
        for c, label in cells:
            p.now(c, label)
    p.now((3, 3, 50), occ=0), p.before((3, 3, 50), word(B))
    return p.case(shape_builds(WORLD_CHANGE_APPEARED, WORLD_CHANGE_VANISHED))


def word_wrap():
    """x of 8 cells at brick offset 0: cx = 7 of one row and cx = 0 of the next are neighbours in a layer word, not in space;
    a pair across the z seam for comparison"""
    cfg = sc.config("C")
    p = Pair("C", steps_at(cfg, (3, -2, 5), (0, 0, 0)), block_occ=0, archive=FREE)
    for c in ((7, 1, 5), (0, 2, 5), (0, 1, 7), (0, 1, 8)):
        p.now(c, B)
    want = dict(n_regions_total=3, n_cells=4)
    return p.case([(dict(), want), (dict(face_connected=True), want)])


# ---- a brick beyond the int16 range: the block straddles brick 32767 | 32768 on x
def beyond_range():
    p = Pair("A", [262143, -262141, 9], block_occ=0, archive=word(B))
    p.now((0, 0, 0), B), p.now((3, 3, 3), R), p.now((1, 2, 3), occ=-1)   # x = 3 lies in brick 32768: that cell is new, not the same
    return p.case([(dict(), dict(n_vanished=3 * 4 * 4 - 2, n_remembered_min=1, n_new_occupied=1, n_new_free=4 * 4 - 1, n_same_occupied=1)),
                   (dict(face_connected=True, by_label=True), dict())])


# ---- OLDER: the bricks archived at stamp 1 are compared, those at stamp 5 are not
def two_stamps():
    cfg = sc.config("A")
    p = Pair("A", steps_at(cfg, (-3, 2, 1), (7, 7, 7)), block_occ=0, archive=word(R))
    for k in itertools.product(range(2), repeat=3):
        p.stamps[tuple(int(v) for v in p.b0 + np.array(k))] = 1 if sum(k) % 2 == 0 else 5
    # the block's one cell of brick b0, then 3, 3, 9, 9, 9 and 27 cells: the even-sum bricks hold 1 + 9 + 9 + 9 of 64
    return p.case([(dict(max_last_stamp=3), dict(n_vanished=28, n_new_free=36)), (dict(max_last_stamp=0), dict(n_vanished=0, n_new_free=64)),
                   (dict(max_last_stamp=5), dict(n_vanished=64)), (dict(), dict(n_vanished=64)),
                   (dict(max_last_stamp=1, by_label=True, face_connected=True), dict(n_vanished=28))])


# ---- random: a block against an edited copy of itself
def random_pair(seed=7):
    cfg = sc.config("B")
    p = Pair("B", sc.crafted_steps(cfg))
    rng = np.random.default_rng(seed)
    shape = p.occ.shape
    p.occ[:] = rng.choice(np.array([-1, 0, 0, 0, 1, 1], np.int8), size=shape)
    lab = rng.choice(np.array([B, R, CAR], np.uint8), size=shape)
    p.label[:] = lab
    for l in (B, R, CAR):
        p.track[lab == l] = TRACK[l]
    own = block_words(dict(occ=p.occ, label=p.label, track=p.track))
    palette = np.array([UNKNOWN, FREE, FREE, word(B), word(R), word(CAR), word(B, occ=2), word(R, track=5), word(CAR, track=synth.TRACK_POLE)], np.uint32)
    p.grid[:] = rng.choice(palette, size=p.grid.shape)                       # the candidates' cells outside the block too
    inside = p.grid[p.inside]
    keep = rng.random(shape) < 0.6
    p.grid[p.inside] = np.where(keep, own, inside)
    bricks = list(itertools.product(*(range(int(n)) for n in p.nb)))
    for i in rng.choice(len(bricks), 6, replace=False):
        p.skip.add(tuple(int(v) for v in p.b0 + np.array(bricks[i])))
    for k in bricks:
        p.stamps[tuple(int(v) for v in p.b0 + np.array(k))] = int(rng.choice([1, 5]))
    builds = every_flag_set() + [(dict(max_last_stamp=3), {}), (dict(max_last_stamp=3, by_label=True, static_only=True), {}),
                                 (dict(min_cells=4), {}), (dict(min_cells=2, face_connected=True, by_label=True), {}),
                                 (dict(classes=(WORLD_CHANGE_VANISHED, WORLD_CHANGE_RELABELLED), labels=(B, CAR)), {}),
                                 (dict(labels=(R,), static_only=True), {})]
    return p.case(builds)


def crafted():
    few = [(dict(), {}), (dict(face_connected=True, by_label=True), {}), (dict(static_only=True, observed_only=True), {})]
    return {"class table": class_table(), "class table at 0": class_table((0, 0, 0), few), "class table at 7": class_table((7, 7, 7), few),
            "vanished shapes": vanished_shapes(), "appeared shapes": appeared_shapes(), "word wrap": word_wrap(),
            "beyond range": beyond_range(), "two stamps": two_stamps()}
