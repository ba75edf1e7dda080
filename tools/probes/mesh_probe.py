"""Times the surface mesh on the C3 map (256^3): prefilled to ~2 M particles (synth.prefill_state) plus a few frames of the
street scene.  For each option set - everything, static only without the faces towards unknown space and the map's ends,
the movable objects alone - one JSON line with
  * the build: the host time of one sdm_mesh_update (it only enqueues) and the time per build of `--iters` builds issued
    back to back and ended by one wait, with the rate at which that reads the second result word of every voxel (4 B x V;
    the 8-byte result is fetched in 64-byte lines either way, so the line traffic is twice that);
  * what the mesh holds: solid cells, faces by direction and kind, vertices, and the default capacity (V / 8) beside them;
  * the time to fetch the lists (sdm_get_mesh_faces + sdm_get_mesh_vertices).
Then what the layer replaces: voxels() and tests/mesh_ref.py on the host (--host-ref).  Kernel times come from a separate
run, without counters, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/mesh_probe.py --iters 5`
(that run also builds the frontiers once per option set: k_frontier_classify reads the same bytes the same way).

  python tools/probes/mesh_probe.py [--iters N] [--frames F] [--host-ref] [--ply PATH]
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
    ap.add_argument("--ply", default=None, help="write the first option set's mesh there, coloured by label")
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
    sets = (("all", dict()), ("static_seen", dict(static_only=True, skip_unknown_faces=True, skip_border_faces=True)),
            ("movable", dict(movable_only=True)))
    for name, kw in sets:
        m.mesh_update(**kw)
        info, _ = m.mesh_info()
        over = bool(info["n_faces"] > info["options"]["max_faces"] or info["n_vertices"] > info["options"]["max_vertices"])
        if over:                                   # the default capacity does not hold this mesh: time the build that does
            kw = dict(kw, max_faces=int(info["n_faces"]), max_vertices=int(info["n_vertices"]))
        host_us, build_us = timed_device(m, lambda: m.mesh_update(**kw), args.iters)
        m.frontiers_update()                       # (the yardstick's kernel, for the kernel trace)
        t0 = time.perf_counter()
        mesh = m.mesh()
        fetch_ms = (time.perf_counter() - t0) * 1e3
        info = mesh["info"]
        print(json.dumps({"mesh": "C3", "options": name, "voxels": V, "iters": args.iters, "host_us_per_update": round(host_us, 1),
                          "us_per_build": round(build_us, 1), "word_bytes": V * 4, "word_TBps": round(V * 4 / build_us / 1e6, 3),
                          "line_TBps": round(V * 8 / build_us / 1e6, 3), "n_solid": int(info["n_solid"]), "n_faces": int(info["n_faces"]),
                          "n_vertices": int(info["n_vertices"]), "faces_by_dir": info["faces_by_dir"].tolist(),
                          "faces_by_kind": info["faces_by_kind"].tolist(), "default_capacity": V // 8, "over_default": over,
                          "fetch_ms": round(fetch_ms, 2)}), flush=True)
        if args.ply and name == "all":
            label = mesh["faces"]["label"].astype(np.int64)
            binding.write_ply(args.ply, mesh["xyz"], mesh["quads"], np.stack([label * 53 % 256, label * 97 % 256, label * 193 % 256], axis=1))
        if args.host_ref:
            from tests import esdf_ref as er
            from tests import mesh_ref as mr
            from tests import query_ref as qr
            t0 = time.perf_counter()
            vox = m.voxels()
            t1 = time.perf_counter()
            geo = qr.Geometry(cfg, m.ring_state())
            f = ((mr.STATIC_ONLY if kw.get("static_only") else 0) | (mr.MOVABLE_ONLY if kw.get("movable_only") else 0) |
                 (mr.SKIP_UNKNOWN_FACES if kw.get("skip_unknown_faces") else 0) | (mr.SKIP_BORDER_FACES if kw.get("skip_border_faces") else 0))
            opt = mr.options(flags=f, max_faces=kw.get("max_faces", 0), max_vertices=kw.get("max_vertices", 0))
            want = mr.build(er.snapshot_grid(geo, vox), cfg["max_movable_track"], opt, cfg["voxel_size"], (geo.center + geo.pmin).astype(np.float32))
            t2 = time.perf_counter()
            equal = all(want[k].tobytes() == mesh[k].tobytes() for k in ("faces", "quads", "corners", "xyz", "info"))
            print(json.dumps({"mesh": "host_replacement_C3", "options": name, "download_ms": round((t1 - t0) * 1e3, 1),
                              "python_ms": round((t2 - t1) * 1e3, 1), "device_us": round(build_us, 1), "equal": bool(equal)}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
