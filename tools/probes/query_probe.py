"""Times the batched map queries (sdm_query_points / _segments / _boxes) in device mode on the C3 map: prefilled to ~2 M
particles (synth.prefill_state) plus a few frames of the street scene.  Host clock around `--iters` back-to-back calls
ended by sdm_synchronize, after warm-up; one JSON line per query with us per call and the cache lines the inputs touch
(computed on the host from the inputs and the host-mode results - upper bounds: a 128-byte line per gathered cell, a
line per cell of a segment's walk, lines per x row of a box).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/query_probe.py --iters 20`.

  python tools/probes/query_probe.py [--iters N] [--frames F]
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
    cam = None
    for t in range(args.frames):
        depth, cloud, pos, q = scene.render(t, params)
        m.update(depth, cloud, pos, q, scene.moves(t))
        cam = np.asarray(pos, np.float32)
    m.synchronize()
    r = m.ring_state()
    size = np.float32(cfg["voxel_size"])
    N = np.array([1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]])
    lo = np.array(r["map_center"], np.float32) - N // 2 * size
    hi = np.array(r["map_center"], np.float32) + N // 2 * size
    rng = np.random.default_rng(1)

    pts = rng.uniform(lo, hi, (1 << 20, 3)).astype(np.float32)
    d = rng.normal(size=(65536, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    a = rng.uniform(lo, hi, (65536, 3))
    seg = np.concatenate([a, a + 20.0 * d], axis=1).astype(np.float32)
    az = np.linspace(-0.8, 0.8, 64)
    el = np.linspace(-0.3, 0.3, 64)
    A, E = np.meshgrid(az, el)
    fan = np.stack([np.sin(A) * np.cos(E), np.sin(E), np.cos(A) * np.cos(E)], axis=-1).reshape(-1, 3)
    rays = np.concatenate([np.broadcast_to(cam, fan.shape), cam + 20.0 * fan], axis=1).astype(np.float32)
    bl = rng.uniform(lo, hi - np.array([1, 1, 2], np.float32), (16384, 3)).astype(np.float32)
    boxes = np.concatenate([bl, bl + np.array([1, 1, 2], np.float32)], axis=1).astype(np.float32)

    # host-mode answers: what the cache-line counts are computed from
    _, idx = m.query_points(pts, with_index=True)
    hs = m.query_segments(seg[:, :3], seg[:, 3:])
    hr = m.query_segments(rays[:, :3], rays[:, 3:])
    ins = idx != 0xFFFFFFFF
    lines_pts = int(ins.sum()) * LINE

    def box_lines(b):
        u0 = np.floor(((b[:, :3] - np.array(r["map_center"], np.float32)) + N // 2 * size) / size)
        u1 = np.floor(((b[:, 3:] - np.array(r["map_center"], np.float32)) + N // 2 * size) / size)
        u0, u1 = np.maximum(u0, 0), np.minimum(u1, N - 1)
        w = np.maximum(u1 - u0 + 1, 0)
        return int((w[:, 1] * w[:, 2] * (np.ceil(w[:, 0] * 8 / LINE) + 1)).sum()) * LINE

    jobs = {
        "points_1M": (lambda x, o: m.query_points(x, on_device=True, n=len(pts), out=o), pts, 8, lines_pts),
        "segments_65536x20m": (lambda x, o: m.query_segments(x, on_device=True, n=len(seg), out=o), seg, 16,
                               int(hs["cells"].sum()) * LINE),
        "rays_4096_fan": (lambda x, o: m.query_segments(x, on_device=True, n=len(rays), out=o), rays, 16, int(hr["cells"].sum()) * LINE),
        "boxes_16384_1x1x2m": (lambda x, o: m.query_boxes(x, on_device=True, n=len(boxes), out=o), boxes, 20, box_lines(boxes)),
    }
    for name, (fn, inp, out_b, lines) in jobs.items():
        x, o = m.device_put(np.ascontiguousarray(inp)), m.device_alloc(len(inp) * out_b)   # (the library's own HBM buffers)
        for _ in range(3):
            fn(x, o)
        m.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn(x, o)
        m.synchronize()
        us = (time.perf_counter() - t0) / args.iters * 1e6
        print(json.dumps({"query": name, "n": len(inp), "us_per_call": round(us, 2), "lines_touched_bytes": lines,
                          "line_bound_us_at_8TBps": round(lines / 8e12 * 1e6, 2), "iters": args.iters,
                          "prefill_particles": int(n_pre)}), flush=True)
        m.device_free(x)
        m.device_free(o)
    m.close()


if __name__ == "__main__":
    main()
