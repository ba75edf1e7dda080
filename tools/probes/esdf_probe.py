"""Times the distance field on the C3 map (256^3): prefilled to ~2 M particles (synth.prefill_state) plus a few frames
of the street scene.  Host clock around `--iters` back-to-back calls ended by sdm_synchronize, after warm-up; one JSON
line for sdm_esdf_update (with the bytes the three passes must move: the x pass reads the 8-byte results and writes
site and snapshot, the y and z passes read and write site) and one for 1 M sdm_query_distance in device mode (with
the cache lines the gathers touch, computed on the host: the 128-byte lines of the point's cell, its eight corners
and its nearest obstacle's snapshot word).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/esdf_probe.py --iters 20`.

  python tools/probes/esdf_probe.py [--iters N] [--frames F]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from semantic_dsp_map_amd import binding, synth  # noqa: E402

LINE = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--frames", type=int, default=4)
    args = ap.parse_args()
    cfg, params = synth.CONFIGS["C3"], synth.PARAMS["vkitti2"]
    scene = synth.Scene(cfg, n_static=48, n_dynamic=6, seed=7)
    st, ring, n_pre = synth.prefill_state(cfg, scene, 2000000)
    m = binding.SdmMap(cfg, params, synth.noise_table())
    m.load_state(st)
    m.set_ring_state(ring)
    for t in range(args.frames):
        depth, cloud, pos, q = scene.render(t, params)
        m.update(depth, cloud, pos, q, scene.moves(t))
    m.synchronize()
    V = m.V
    n_occ = int((m.voxels()["occ"] >= 1).sum())

    def timed(fn):
        for _ in range(3):
            fn()
        m.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        m.synchronize()
        return (time.perf_counter() - t0) / args.iters * 1e6

    us = timed(m.esdf_update)
    build_bytes = V * 8 + V * 8 + 2 * (V * 4 + V * 4)
    print(json.dumps({"esdf": "update_C3", "voxels": V, "obstacles": n_occ, "us_per_call": round(us, 2),
                      "bytes": build_bytes, "byte_bound_us_at_6TBps": round(build_bytes / 6e12 * 1e6, 2),
                      "iters": args.iters, "prefill_particles": int(n_pre)}), flush=True)

    d2, site, origin = m.esdf()
    size = np.float32(cfg["voxel_size"])
    N = np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]])
    rng = np.random.default_rng(1)
    pts = rng.uniform(origin, origin + N * size, (1 << 20, 3)).astype(np.float32)
    # cache lines of the gathers (host-side count: the site words of the cell and its corners, the snapshot word)
    u = (pts - origin) / size
    c0 = np.clip(np.floor(u - 0.5), 0, N - 1).astype(np.int64)
    c1 = np.clip(np.floor(u - 0.5) + 1, 0, N - 1).astype(np.int64)
    lines = set()
    for by in (0, 1):
        for bz in (0, 1):
            for cx in (c0[:, 0], c1[:, 0]):
                y, z = (c1 if by else c0)[:, 1], (c1 if bz else c0)[:, 2]
                lines.update(((cx + N[0] * (y + N[1] * z)) * 4 // LINE).tolist())
    sites = site.reshape(-1)[(np.floor(u[:, 0]) + N[0] * (np.floor(u[:, 1]) + N[1] * np.floor(u[:, 2]))).astype(np.int64)]
    snap_lines = len(set((sites[sites != 0xFFFFFFFF].astype(np.int64) * 4 // LINE).tolist()))
    touched = (len(lines) + snap_lines) * LINE + len(pts) * (12 + 36)
    x, o = m.device_put(pts), m.device_alloc(len(pts) * 36)
    us = timed(lambda: m.query_distance(x, on_device=True, n=len(pts), out=o))
    print(json.dumps({"esdf": "query_distance_1M", "n": len(pts), "us_per_call": round(us, 2), "lines_touched_bytes": touched,
                      "line_bound_us_at_6TBps": round(touched / 6e12 * 1e6, 2), "iters": args.iters}), flush=True)
    m.device_free(x)
    m.device_free(o)
    m.close()


if __name__ == "__main__":
    main()
