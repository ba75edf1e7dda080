"""Z-slab shardings that sdm_create accepts and the rest of the suite does not build: slabs of one or two planes, shards
of fewer voxels than one 64-voxel chunk or one 512-voxel group, shards that own no pixel of the ck image.  Plain numpy,
importable without a GPU: the (grid, G) cases with the property each one is there for, the shard geometry restated from
sdm_create (csrc/lifecycle.hip), and the crafted state of an object larger than one shard."""
import numpy as np

from semantic_dsp_map_amd import synth
from tests import shape_cases as sc

# the T0 grid seen by a camera of 48 x 40 pixels: 1920 pixels in chunks of 64 at G = 32, shards 30 and 31 own only padding
SMALL_CAMERA = dict(width=48, height=40, fx=30.0, fy=30.0, cx=24.0, cy=20.0)

# name: grid (a shape case of shape_cases, "T0" or "T0cam"), G, and what the case is there for
#   planes: z planes per slab; vox: "lt64" / "lt512" / "eq512" / "ge512" voxels per shard; empty_ck: shards owning no pixel
CASES = {
    "T0/8": dict(grid="T0", G=8, planes=4, vox="ge512", empty_ck=()),
    "T0/16": dict(grid="T0", G=16, planes=2, vox="ge512", empty_ck=()),
    "T0/32": dict(grid="T0", G=32, planes=1, vox="ge512", empty_ck=()),            # one plane per slab
    "A/4": dict(grid="A", G=4, planes=1, vox="lt64", empty_ck=()),                 # 16 voxels: less than one chunk
    "B/16": dict(grid="B", G=16, planes=4, vox="eq512", empty_ck=()),              # one group per shard
    "B/32": dict(grid="B", G=32, planes=2, vox="lt512", empty_ck=()),              # half a group
    "C/32": dict(grid="C", G=32, planes=4, vox="lt512", empty_ck=()),              # two chunks, 16 slots
    "D/8": dict(grid="D", G=8, planes=1, vox="ge512", empty_ck=()),                # y of 512, seen edge-on by the tilted camera
    "T0cam/32": dict(grid="T0cam", G=32, planes=1, vox="ge512", empty_ck=(30, 31)),  # ck chunks wholly beyond the image
}
SHAPE_CASES = ["A/4", "B/16", "B/32", "C/32", "D/8"]     # the shape cases, driven by shape_cases.drive
SWEEP_CASES = ["B/16", "B/32", "C/32", "A/4"]            # the non-incremental sweeps on shards
MAX_LIVE_SHARDS = 32                                      # shard maps alive in one process at once


def config(name):
    grid = CASES[name]["grid"]
    if grid == "T0":
        return dict(synth.CONFIGS["T0"])
    if grid == "T0cam":
        return dict(synth.CONFIGS["T0"], **SMALL_CAMERA)
    return sc.config(grid)


def shape_of(name):
    """the shape_cases name the case drives (T0 and T0cam: None)"""
    grid = CASES[name]["grid"]
    return grid if grid in sc.CASES else None


def sdm_create_accepts_shard(cfg, rank, G):
    """sdm_create's rules on the grid and the sharding (csrc/lifecycle.hip), restated"""
    return sc.sdm_create_accepts(cfg) and G >= 1 and 0 <= rank < G and (1 << cfg["z_n"]) % G == 0


def planes(cfg, G):
    return (1 << cfg["z_n"]) // G


def v_count(cfg, G):
    return (1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])) // G


def vox_class(n):
    return "lt64" if n < 64 else "lt512" if n < 512 else "eq512" if n == 512 else "ge512"


def ck_chunk(cfg, G):
    """pixels of the ck image per shard: ceil(H W / G) rounded up to 64 (sdm_ck_chunk_elems)"""
    hw = cfg["width"] * cfg["height"]
    return -(-(-(-hw // G)) // 64) * 64


def ck_empty_shards(cfg, G):
    """shards whose chunk lies wholly beyond the image (only padding)"""
    hw = cfg["width"] * cfg["height"]
    return tuple(k for k in range(G) if k * ck_chunk(cfg, G) >= hw)


def slab_of(cfg, G, voxel):
    """the shard owning storage voxel `voxel` (ring-z slab)"""
    rz = np.asarray(voxel, np.int64) >> (cfg["x_n"] + cfg["y_n"])
    return rz // planes(cfg, G)


# ---- an object larger than one shard (T0)
BIG_TRACK = 3                  # movable (<= max_movable_track), a car
BIG_BLOCK = (16, 16, 10)       # cells (x, y, z) of its block; slots 1-7 of each cell hold a member: 17920 members
BIG_SLOTS = 7
BIG_DZ = 5                     # the frame moves it about this many planes up z ...
BIG_YAW = 0.1                  # ... turning it by this much (radians) about its centre


def big_ring(cfg):
    """the crafted ring of shape_cases (shifted on every axis) - on T0, map z = ring z - 17 (mod 32)"""
    return sc.crafted_ring(cfg, sc.crafted_steps(cfg))


def big_block(cfg, ring):
    """map cells (x, y, z) of the block: its ring z planes run 24 .. 33 (mod 32) - across the ring's z wrap, and so are
    the planes it moves into"""
    geo_eq = int(ring["eq_steps"][2])
    NZ = 1 << cfg["z_n"]
    z0 = (24 - geo_eq) % NZ
    x, y, z = np.meshgrid(np.arange(8, 8 + BIG_BLOCK[0]), np.arange(8, 8 + BIG_BLOCK[1]), np.arange(z0, z0 + BIG_BLOCK[2]),
                          indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def big_state(cfg, ring):
    cells = big_block(cfg, ring)
    return sc.crafted_state(cfg, ring, cells, tracks=np.full(len(cells), BIG_TRACK, np.uint16),
                            labels=np.full(len(cells), synth.LABEL_CAR, np.uint8), owner=BIG_TRACK, slots=BIG_SLOTS)


def big_move(cfg, ring):
    """the frame's move of the object: a turn of BIG_YAW about the y axis through the block's centre, then BIG_DZ planes up"""
    from tests.test_fuzz_gpu import rot_y
    size = np.float32(cfg["voxel_size"])
    N = np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.float64)
    cells = big_block(cfg, ring)
    pmin = -(N / 2) * float(size) + np.array(ring["map_center"], np.float64)
    c = pmin + (cells.min(0) + cells.max(0) + 1) / 2.0 * float(size)
    R = rot_y(BIG_YAW)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R.astype(np.float32)
    T[:3, 3] = (c - R @ c + np.array([0.0, 0.0, BIG_DZ * float(size)])).astype(np.float32)
    mv = np.zeros(1, synth.OBJECT_MOVE)
    mv[0]["track_id"], mv[0]["T"] = BIG_TRACK, T.reshape(-1)
    return mv
