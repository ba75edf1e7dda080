"""Times the instance table on the C3 map (256^3): prefilled to ~2 M particles (synth.prefill_state) plus a few frames
of the street scene, and on a fresh map of the same size (no counted cell: the streaming pass alone).  Host clock around
`--iters` back-to-back sdm_instances_update calls ended by one sdm_synchronize, after warm-up; one JSON line per map
with the bytes the pass must read (the 8-byte results, once).  For the record, what the table replaces: voxels() plus
tests/instances_ref.py on the same map (--host-ref).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/instances_probe.py --iters 20`.

  python tools/probes/instances_probe.py [--iters N] [--frames F] [--host-ref]
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
    for _ in range(3):
        fn()
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    m.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


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
    bound = round(V * 8 / 6e12 * 1e6, 2)
    for movable_only in (False, True):
        us = timed(m, lambda: m.instances_update(movable_only=movable_only), args.iters)
        table, _ = m.instances()
        top = np.sort(table["n_cells"])[::-1][:3].tolist()
        print(json.dumps({"instances": "update_C3", "movable_only": movable_only, "voxels": V, "instances_n": len(table),
                          "counted_cells": int(table["n_cells"].sum()), "largest": top, "us_per_call": round(us, 2), "bytes": V * 8,
                          "byte_bound_us_at_6TBps": bound, "iters": args.iters, "prefill_particles": int(n_pre)}), flush=True)
    if args.host_ref:
        from tests import instances_ref as ir
        from tests import query_ref as qr
        t0 = time.perf_counter()
        vox = m.voxels()
        t1 = time.perf_counter()
        ref = ir.instances(qr.Geometry(cfg, m.ring_state()), vox, cfg["max_movable_track"], cfg["voxel_size"], 0)
        t2 = time.perf_counter()
        m.instances_update()
        table, _ = m.instances()
        print(json.dumps({"instances": "host_replacement_C3", "download_ms": round((t1 - t0) * 1e3, 1), "numpy_ms": round((t2 - t1) * 1e3, 1),
                          "equal": ir.equal_tables(table, ref) is None}), flush=True)
    m.close()
    fresh = binding.SdmMap(cfg, params, synth.noise_table())
    us = timed(fresh, fresh.instances_update, args.iters)
    print(json.dumps({"instances": "update_C3_fresh", "voxels": V, "instances_n": len(fresh.instances()[0]), "us_per_call": round(us, 2),
                      "byte_bound_us_at_6TBps": bound, "iters": args.iters}), flush=True)
    fresh.close()


if __name__ == "__main__":
    main()
