"""Times the frontier build on the C3 map (256^3): prefilled to ~2 M particles (synth.prefill_state) plus a few frames of
the street scene, and on a fresh map of the same size (no free cell: the classification pass, the mask and the scans
alone).  Host clock around `--iters` back-to-back sdm_frontiers_update calls ended by one sdm_synchronize, after warm-up;
one JSON line per map and connectivity with the number of frontier cells and clusters and the bytes the build must move
(the 8-byte results once, the bitmasks written and read, the cell list's arrays).  In the same run, what the build
replaces: voxels() plus tests/frontiers_ref.py on the same map (--host-ref).  Kernel times come from a separate run,
without counters, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/frontiers_probe.py --iters 20`.

  python tools/probes/frontiers_probe.py [--iters N] [--frames F] [--host-ref]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_dsp_map_amd import binding, synth  # noqa: E402


def timed(m, fn, iters):
    for _ in range(3):
        fn()
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    m.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def must_move(V, n_cells):
    """bytes: the results once; three bitmasks written, the unknown mask read 7 times over and the other two once or
    twice (all of it L2-sized); the words' counts written, scanned and read; per cell its list entries and accumulator"""
    return V * 8 + (V // 8) * 6 + (V // 64) * 4 * 4 + n_cells * (4 * 6 + 1 + 56 * 2)


def report(tag, m, V, iters, **extra):
    import ctypes as C
    max_cells = 0   # the default capacity, V / 16; a map with more frontier cells is timed again with a list of their number
    for face in (True, False):
        us = timed(m, lambda: m.frontiers_update(face_connected=face, max_cells=max_cells), iters)
        n64 = C.c_int64(0)
        if m.L.sdm_get_frontier_cells(m.h, None, None, None, 0, C.byref(n64)) == 4:   # SDM_ERR_CAPACITY
            max_cells = n64.value
            us = timed(m, lambda: m.frontiers_update(face_connected=face, max_cells=max_cells), iters)
        extra["max_cells"] = max_cells or V // 16
        table, _ = m.frontiers()
        cell, cluster, faces = m.frontier_cells()
        n = len(cell)
        top = sorted(table["n_cells"].tolist(), reverse=True)[:3]
        by = must_move(V, n)
        print(json.dumps(dict({"frontiers": tag, "face_connected": face, "voxels": V, "frontier_cells": n, "clusters": len(table),
                               "largest": top, "us_per_call": round(us, 2), "bytes": by, "byte_bound_us_at_6TBps": round(by / 6e12 * 1e6, 2),
                               "results_only_us_at_6TBps": round(V * 8 / 6e12 * 1e6, 2), "iters": iters}, **extra)), flush=True)


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
    V = m.V
    report("update_C3", m, V, args.iters, prefill_particles=int(n_pre))
    if args.host_ref:
        from tests import frontiers_ref as fr
        from tests import query_ref as qr
        t0 = time.perf_counter()
        vox = m.voxels()
        t1 = time.perf_counter()
        ref = fr.frontiers(qr.Geometry(cfg, m.ring_state()), vox, cfg["voxel_size"])
        t2 = time.perf_counter()
        m.frontiers_update()
        print(json.dumps({"frontiers": "host_replacement_C3", "download_ms": round((t1 - t0) * 1e3, 1), "numpy_ms": round((t2 - t1) * 1e3, 1),
                          "equal": fr.equal_all(m.frontiers()[0], m.frontier_cells(), ref) is None}), flush=True)
    m.close()
    fresh = binding.SdmMap(cfg, params, synth.noise_table())
    report("update_C3_fresh", fresh, V, args.iters)
    fresh.close()


if __name__ == "__main__":
    main()
