"""Map shapes that sdm_create accepts and the rest of the suite does not build: axes of 4 cells, x rows of 4 and 8 cells,
maps smaller than one 512-voxel group, axes of 512 cells on non-cubic maps.  Plain numpy, importable without a GPU: the
cases, their configurations (the T0 camera), a free-running camera path over random_frame's frames, the float32
restatement of the emitted positions, and a builder of crafted states (chosen cells occupied / free / unknown on a
shifted ring) for load_state."""
import numpy as np

from semantic_dsp_map_amd import synth
from tests import query_ref as qr
from tests.test_fuzz_gpu import random_frame, rot_y

# name: (x_n, y_n, z_n, p_n), voxel size, tilt of the camera about the x axis (radians; -pi/2 looks along +y)
CASES = {
    "A": dict(n=(2, 2, 2, 1), voxel_size=1.0, tilt=0.0),     # 64 voxels: less than one group, one sweep tile, one emit tile
    "B": dict(n=(2, 5, 6, 3), voxel_size=0.25, tilt=0.0),    # x of 4 cells on a map of many groups
    "C": dict(n=(3, 2, 7, 4), voxel_size=0.3, tilt=0.0),     # a group is one row, y of 4 cells, 16 slots
    "D": dict(n=(4, 9, 3, 2), voxel_size=0.25, tilt=-np.pi / 2),   # y of 512 (k_esdf_env<1>, 128 KB of LDS), x_n < 6
    "E": dict(n=(9, 3, 9, 1), voxel_size=0.1, tilt=0.0),     # x and z of 512: k_esdf_x's 8 chunks, k_esdf_env<2>, 2 M voxels
    "F": dict(n=None, voxel_size=None, tilt=0.0),            # REF_ZED2_BOOST's grid (the shipped one)
}
PARITY_CASES = ["A", "B", "C", "D", "E"]
ALL_CASES = PARITY_CASES + ["F"]


def config(name):
    c = CASES[name]
    cfg = dict(synth.CONFIGS["T0"])
    if c["n"] is None:
        ref = synth.CONFIGS["REF_ZED2_BOOST"]
        cfg.update(x_n=ref["x_n"], y_n=ref["y_n"], z_n=ref["z_n"], p_n=ref["p_n"], voxel_size=ref["voxel_size"])
    else:
        x_n, y_n, z_n, p_n = c["n"]
        cfg.update(x_n=x_n, y_n=y_n, z_n=z_n, p_n=p_n, voxel_size=c["voxel_size"])
    return cfg


def sdm_create_accepts(cfg):
    """sdm_create's rules on the grid (csrc/lifecycle.hip), restated"""
    n = [cfg["x_n"], cfg["y_n"], cfg["z_n"]]
    return (sum(n) + cfg["p_n"] <= 31 and all(2 <= v <= 9 for v in n) and 1 <= cfg["p_n"] <= 4 and cfg["voxel_size"] > 0
            and cfg["width"] > 0 and cfg["height"] > 0 and 0 <= cfg["window_half"] <= 7)


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def mat_quat(R):
    """(w, x, y, z) of a rotation matrix (Hamilton; yaw_quat(t) for rot_y(t))"""
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.array(q, np.float64)
    return q if q[0] >= 0 else -q


def quat_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def drive(name, params, n_frames, seed, cfg=None):
    """random_frame's frames for case `name` on a free-running camera: steps of about one voxel on every axis (the ring
    follows the camera cell by cell, both ways), and at n_frames // 2 one jump of more than half the map on every axis.
    `cfg` (name None): another grid and camera, untilted.  Yields (t, depth, cloud, pos float32, q float32, moves, remove)."""
    tilt = CASES[name]["tilt"] if name is not None else 0.0
    cfg = config(name) if cfg is None else cfg
    T = rot_x(tilt)
    rng = np.random.default_rng(seed)
    size = cfg["voxel_size"]
    N = np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.float64)
    pos, yaw = np.zeros(3), 0.0
    for t in range(n_frames):
        pos = pos + rng.normal(0, 0.9 * size, 3)
        if t == n_frames // 2:
            pos = pos + (N // 2 + 3) * size * np.array([1.0, -1.0, 1.0])
        yaw += rng.normal(0, 0.08)
        depth, cloud, mv, remove = random_frame(rng, cfg, params, t, pos, yaw)
        if tilt:
            valid = cloud["is_valid"] != 0
            p = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float64)
            p = (p - pos) @ T.T + pos
            cloud["x"], cloud["y"], cloud["z"] = np.where(valid[:, None], p, 0).T
        q = mat_quat(T @ rot_y(yaw)).astype(np.float32)
        yield t, depth, cloud, pos.astype(np.float32), q, mv, remove


def emit_positions(cfg, ring, voxel, sub=(0.0, 0.0, 0.0)):
    """the min corner of storage voxels `voxel` as the emitted clouds give it (kernels.hip emit_voxel_corner), float32:
    ring index -> map index (axis_correct of r - eq) -> m * size + pmin, + the frame's centre, - sub"""
    n_bits = [cfg["x_n"], cfg["y_n"], cfg["z_n"]]
    N = [1 << b for b in n_bits]
    v = np.asarray(voxel, np.int64)
    r = [v & (N[0] - 1), (v >> n_bits[0]) & (N[1] - 1), v >> (n_bits[0] + n_bits[1])]
    size = np.float32(cfg["voxel_size"])
    out = []
    for a in range(3):
        m = r[a] - int(ring["eq_steps"][a])
        m = np.where(m < 0, m + N[a], np.where(m >= N[a], m - N[a], m))
        pmin = -(np.float32(N[a] >> 1) * size)
        c = (m.astype(np.float32) * size + pmin).astype(np.float32)
        c = (c + np.float32(ring["map_center"][a])).astype(np.float32)
        out.append((c - np.float32(sub[a])).astype(np.float32))
    return np.stack(out, 1)


# ---- crafted states
GTS = 3             # global time stamp of a crafted state: every cell observed at it unless it is to read unknown
W_OBSTACLE = 60.0   # an obstacle's particle weight: still above the threshold after a frame's missed detection in view (x 0.02)
ST_TIMEPTC, ST_UPDATED = 5, 1


def crafted_ring(cfg, steps):
    """a ring state moved by `steps` cells per axis from the origin: eq = steps mod N (signed, as the map keeps it), the
    camera in the middle of the cell the ring follows (its next frame moves nothing)"""
    size = np.float32(cfg["voxel_size"])
    N = [1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]]
    eq = [int(np.sign(s)) * (abs(int(s)) % N[a]) for a, s in enumerate(steps)]
    centre = [float(np.float32(s) * size) for s in steps]
    cam = [float(np.float32(s + (0.5 if s >= 0 else -0.5)) * size) for s in steps]
    return dict(global_time_stamp=GTS, moved_steps=[int(s) for s in steps], eq_steps=eq, map_center=centre, last_pos=cam,
                birth_cursor=0, move_cursor=0)


def crafted_state(cfg, ring, occupied=(), unknown=(), tracks=None, labels=None, owner=None, slots=1):
    """a state for load_state: every cell observed and free (slot 0 stamped at GTS), except the map cells `unknown`
    (never observed: occ -1) and `occupied` (a particle of weight W_OBSTACLE in each of slots 1 .. `slots`, track / label
    per cell, default a static building; `owner`: the track whose object set holds them, default none).  Cells are
    (x, y, z) map indices; they are placed with query_ref.Geometry.voxel."""
    from semantic_dsp_map_amd import binding
    geo = qr.Geometry(cfg, ring)
    S = 1 << cfg["p_n"]
    V = 1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])
    st = {k: np.zeros(V * S, dt) for k, dt in binding.STATE_FIELDS}
    st["owner"][:] = 0xFFFF
    st["status"][0::S] = ST_TIMEPTC
    st["ts"][0::S] = GTS
    size = np.float32(cfg["voxel_size"])
    unknown = np.asarray(unknown, np.int64).reshape(-1, 3)
    if len(unknown):
        st["ts"][geo.voxel(unknown).astype(np.int64) * S] = 0
    occupied = np.asarray(occupied, np.int64).reshape(-1, 3)
    if len(occupied):
        p = (geo.center + geo.pmin) + (occupied.astype(np.float32) + np.float32(0.5)) * size   # the cell's centre
        for slot in range(1, slots + 1):
            idx = geo.voxel(occupied).astype(np.int64) * S + slot
            st["status"][idx] = ST_UPDATED
            st["w"][idx] = W_OBSTACLE
            st["ts"][idx] = GTS
            st["track"][idx] = synth.TRACK_BUILDING if tracks is None else tracks
            st["label"][idx] = synth.LABEL_BUILDING if labels is None else labels
            st["px"][idx], st["py"][idx], st["pz"][idx] = p[:, 0], p[:, 1], p[:, 2]
            if owner is not None:
                st["owner"][idx] = owner
    return st


def crafted_steps(cfg):
    """ring offsets for crafted states: N - 1 on x, -(N - 1) on y, a few turns and a half on z"""
    N = [1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]]
    return [N[0] - 1, -(N[1] - 1), 2 * N[2] + N[2] // 2 + 1]


def patterns(cfg, ring):
    """crafted obstacle patterns: name -> (occupied cells, unknown cells, tracks or None) in map indices (x, y, z)"""
    N = np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]], np.int64)
    long_ax = int(np.argmax(N))
    out = {}
    out["corner"] = (np.array([[0, 0, 0]]), np.zeros((0, 3)), None)
    out["opposite_corners"] = (np.array([[0, 0, 0], N - 1]), np.zeros((0, 3)), None)
    line = np.zeros((N[long_ax], 3), np.int64)
    line[:, long_ax] = np.arange(N[long_ax])
    line[:, (long_ax + 1) % 3] = N[(long_ax + 1) % 3] // 2
    out["full_line"] = (line, np.zeros((0, 3)), None)
    alt = np.zeros((N[long_ax] // 2, 3), np.int64)
    alt[:, long_ax] = np.arange(0, N[long_ax], 2)
    alt[:, (long_ax + 2) % 3] = N[(long_ax + 2) % 3] - 1
    out["alternate"] = (alt, np.zeros((0, 3)), None)
    # next to the ring's wrap point on every axis: the map cells whose ring index is 0 or N - 1
    geo = qr.Geometry(cfg, ring)
    wrap = (N - geo.eq) % N
    near = []
    for a in range(3):
        for c in (wrap[a] - 1, wrap[a]):
            cell = N // 3
            cell[a] = c % N[a]
            near.append(cell.copy())
    out["wrap"] = (np.unique(np.array(near), axis=0), np.zeros((0, 3)), None)
    # unknown cells only (obstacles under UNKNOWN_IS_OBSTACLE), a pair of them far apart
    out["unknown_only"] = (np.zeros((0, 3), np.int64), np.array([N // 4, N - 1 - N // 5]), None)
    # movable and static tracks (STATIC_ONLY drops the movable ones)
    mix = np.array([[0, N[1] - 1, 0], N // 2, [N[0] - 1, 0, N[2] - 1]], np.int64)
    out["tracks"] = (mix, np.zeros((0, 3)), np.array([3, synth.TRACK_BUILDING, 17], np.uint16))
    return out
