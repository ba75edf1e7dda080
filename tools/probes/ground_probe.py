"""Times the ground layer on the C3 map (256^3): prefilled to ~2 M particles (synth.prefill_state) plus a few frames of the
street scene.  For each up axis - x as (0, +1), y as the scenes have it (1, -1), z as (2, +1) - one JSON line with
  * the build: the host time of one sdm_ground_update (it only enqueues) and the time per build of `--iters` builds
    issued back to back and ended by one wait, with the rate at which that reads the second result word of every voxel
    (4 B x V; the 8-byte result is fetched in 64-byte lines either way, so the line traffic is twice that) beside the
    5.5 TB/s k_esdf_x reaches on the same kind of read;
  * 1 M point queries and 16 K footprints of 4 m x 2 m at random headings, on the device;
  * what the layer holds: the classes' counts.
Then what the layer replaces: voxels() and tests/ground_ref.py on the host (--host-ref).  Kernel times come from a
separate run, without counters, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/ground_probe.py --iters 5`.

  python tools/probes/ground_probe.py [--iters N] [--frames F] [--host-ref]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_dsp_map_amd import binding, synth  # noqa: E402

ESDF_X_TBPS = 5.5   # k_esdf_x on the same map


def timed_device(m, fn, iters):
    for _ in range(2):
        fn()
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()
    m.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) / iters * 1e6, (t2 - t0) / iters * 1e6   # host time per call, time per call to the end of the work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--host-ref", action="store_true")
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
    size, V = cfg["voxel_size"], m.V
    labels = [synth.LABEL_ROAD, synth.LABEL_BUILDING]
    rng = np.random.default_rng(1)
    for up in ((0, 1), (1, -1), (2, 1)):
        N = 1 << cfg[("x_n", "y_n", "z_n")[up[0]]]
        kw = dict(up=up, h_lo=0, h_hi=N - 1, clearance=int(np.ceil(1.8 / size)), max_step=1, support_labels=labels)
        host_us, build_us = timed_device(m, lambda: m.ground_update(**kw), args.iters)
        cells, d2, info, origin = m.ground()
        au, av = [a for a in (0, 1, 2) if a != up[0]]
        pts = (origin + rng.uniform(0, N * size, (1 << 20, 3))).astype(np.float32)
        d_pts, d_out = m.device_put(pts), m.device_alloc((1 << 20) * 32)
        _, us_q = timed_device(m, lambda: m.query_ground(d_pts, on_device=True, n=1 << 20, out=d_out), 10)
        fps = np.zeros(16384, binding.FOOTPRINT)
        th = rng.uniform(0, 2 * np.pi, len(fps))
        fps["center_u"], fps["center_v"] = origin[au] + rng.uniform(0, N * size, len(fps)), origin[av] + rng.uniform(0, N * size, len(fps))
        fps["dir_u"], fps["dir_v"], fps["half_len"], fps["half_wid"] = np.cos(th), np.sin(th), 2.0, 1.0
        d_fps, d_res = m.device_put(fps), m.device_alloc(len(fps) * 32)
        _, us_f = timed_device(m, lambda: m.query_footprints(d_fps, on_device=True, n=len(fps), out=d_res), 10)
        res = m.device_download(d_res, len(fps) * 32, binding.FOOTPRINT_RESULT)
        for p in (d_pts, d_out, d_fps, d_res):
            m.device_free(p)
        print(json.dumps({"ground": "C3", "up": list(up), "voxels": V, "columns": int(cells.size), "iters": args.iters,
                          "host_us_per_update": round(host_us, 1), "us_per_build": round(build_us, 1),
                          "word_bytes": V * 4, "word_TBps": round(V * 4 / build_us / 1e6, 3), "line_TBps": round(V * 8 / build_us / 1e6, 3),
                          "esdf_x_TBps": ESDF_X_TBPS, "us_per_1M_points": round(us_q, 1), "us_per_16K_footprints": round(us_f, 1),
                          "mean_footprint_columns": round(float(res["n_cols"].mean()), 1), "footprints_with_lethal": int((res["n_lethal"] > 0).sum()),
                          "n_ground": int(info["n_ground"]), "n_obstacle": int(info["n_obstacle"]), "n_none": int(info["n_none"]),
                          "n_step": int(info["n_step"]), "n_lethal": int(info["n_lethal"]), "clearance": kw["clearance"]}), flush=True)
        if args.host_ref:
            from tests import esdf_ref as er
            from tests import ground_ref as gr
            from tests import query_ref as qr
            t0 = time.perf_counter()
            vox = m.voxels()
            t1 = time.perf_counter()
            geo = qr.Geometry(cfg, m.ring_state())
            opt = gr.options(up, 0, N - 1, kw["clearance"], 1, labels)
            want_cells, want_d2, _ = gr.build(er.snapshot_grid(geo, vox), cfg["max_movable_track"], opt)
            t2 = time.perf_counter()
            print(json.dumps({"ground": "host_replacement_C3", "up": list(up), "download_ms": round((t1 - t0) * 1e3, 1),
                              "python_ms": round((t2 - t1) * 1e3, 1), "device_us": round(build_us, 1),
                              "equal": bool(want_cells.tobytes() == cells.tobytes() and np.array_equal(want_d2, d2))}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
