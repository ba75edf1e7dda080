"""Times the forecast on the C3 map (256^3): prefilled to ~2 M particles (synth.prefill_state) plus a few frames of the street
scene.  The motions go to the movable tracks with the most cells (the instance table says which), then to track ids that
own no cell, at 1 to 3 m/s: 1 / 8 / 64 motions, 4 and 16 horizons up to 4 s, plain and swept.  sdm_forecast_update does not
wait, so a build is timed on the host clock round `--iters` builds and one synchronize; one JSON line per combination with
the stamps, the sources, the marks, the bytes of the result array (the first yardstick is the time of one pass over it:
k_frontier_classify's, which is in the same trace because the probe builds the frontiers `--iters` times too) and the
bytes k_forecast_classify reads and writes (4 B gathered per result, 8 B written).  Then 65,536
point-time queries and 16,384 space-time segments on the device, and the second yardstick: what the build replaces,
voxels() plus tests/forecast_ref.py on the same map (--host-ref).  Times by kernel come from a separate run, without
counters, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/forecast_probe.py --iters 3`.

  python tools/probes/forecast_probe.py [--iters N] [--frames F] [--host-ref]
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


def timed(m, fn, iters):
    for _ in range(2):
        fn()
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    m.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def motions_for(m, cfg, n, seed=1):
    """n motions: the movable tracks with the most cells first, then ids that own no cell"""
    m.instances_update(movable_only=True)
    table, _ = m.instances()
    have = table["track"][np.argsort(-table["n_cells"].astype(np.int64), kind="stable")][:n]
    spare = [t for t in range(1, cfg["max_movable_track"]) if t not in set(have.tolist())][:n - len(have)]
    mo = np.zeros(n, binding.MOTION)
    mo["track"] = np.concatenate([have, np.array(spare, np.uint16)])
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, 3))
    mo["v"] = (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(1, 3, (n, 1))).astype(np.float32)
    return mo, int(table["n_cells"][np.isin(table["track"], have)].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
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
    for _ in range(args.iters):   # (k_frontier_classify, the one-pass yardstick, in the same trace)
        m.frontiers_update()
    m.synchronize()
    V = m.V
    horizons = {4: np.array([0.5, 1, 2, 4], np.float32), 16: np.arange(1, 17, dtype=np.float32) * 0.25}
    for n in (1, 8, 64):
        mo, cells = motions_for(m, cfg, n)
        for n_h, t in horizons.items():
            for swept in (False, True):
                us = timed(m, lambda: m.forecast_update(mo, t, swept), args.iters)
                info = m.forecast()[2]
                print(json.dumps({"forecast": "update_C3", "voxels": V, "motions": n, "horizons": n_h, "swept": swept, "us_per_build": round(us, 1),
                                  "n_stamps": int(info["n_stamps"]), "n_sources": int(info["n_sources"]), "n_marked": int(info["n_marked"]),
                                  "n_marks_in": int(info["n_marks_in"]), "n_marks_out": int(info["n_marks_out"]),
                                  "result_array_bytes": V * 8, "classify_bytes_read_and_written": V * 4 + V * 8,
                                  "iters": args.iters}), flush=True)
    # queries on the device, on the last build (64 motions, 16 horizons, swept)
    origin = m.forecast()[3]
    rng = np.random.default_rng(1)
    size = cfg["voxel_size"]
    pts = np.concatenate([origin + rng.uniform(0, 256 * size, (65536, 3)), rng.uniform(0, 4, (65536, 1))], axis=1).astype(np.float32)
    a = origin + rng.uniform(0, 256 * size, (16384, 3))
    b = a + rng.normal(0, 20 * size, (16384, 3))
    ta = rng.uniform(0, 2, (16384, 1))
    seg = np.concatenate([a, ta, b, ta + rng.uniform(0, 2, (16384, 1))], axis=1).astype(np.float32)
    d_pts, d_res = m.device_put(pts), m.device_alloc(65536 * 8)
    d_seg, d_hit = m.device_put(seg), m.device_alloc(16384 * 16)
    us_q = timed(m, lambda: m.query_forecast(d_pts, on_device=True, n=65536, out=d_res), args.iters)
    us_s = timed(m, lambda: m.query_forecast_segments(d_seg, on_device=True, n=16384, out=d_hit), args.iters)
    us_cells = timed(m, lambda: m.forecast_cells(), 3)
    hit = m.device_download(d_hit, 16384 * 16, binding.FORECAST_HIT)
    print(json.dumps({"forecast": "queries_C3", "points": 65536, "us_per_point_call": round(us_q, 1), "segments": 16384,
                      "us_per_segment_call": round(us_s, 1), "blocked": int((hit["t"] >= 0).sum()), "mean_cells": round(float(hit["cells"].mean()), 1),
                      "us_per_cell_list": round(us_cells, 1)}), flush=True)
    if args.host_ref:
        from tests import forecast_ref as fc
        from tests import query_ref as qr
        geo = qr.Geometry(cfg, m.ring_state())
        for n, swept in ((8, False), (8, True)):
            mo, _ = motions_for(m, cfg, n)
            t = horizons[4]
            t0 = time.perf_counter()
            vox = m.voxels()
            t1 = time.perf_counter()
            ref = fc.Field(geo, vox, size, mo, t, swept)
            t2 = time.perf_counter()
            us = timed(m, lambda: m.forecast_update(mo, t, swept), args.iters)
            mask, first, info, _ = m.forecast()
            print(json.dumps({"forecast": "host_replacement_C3", "motions": n, "horizons": 4, "swept": swept, "download_ms": round((t1 - t0) * 1e3, 1),
                              "python_ms": round((t2 - t1) * 1e3, 1), "device_us": round(us, 1),
                              "equal": fc.equal_fields(mask, first, info, ref) is None}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
