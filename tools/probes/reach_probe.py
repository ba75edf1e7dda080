"""Times the travel-cost field on the C3 map (256^3): prefilled to ~2 M particles (synth.prefill_state) plus a few frames of
the street scene, the start at the camera - or, where the camera's cell is not traversable under a combination's rule, at the
traversable cell nearest to it (every line says how far the start was moved).  sdm_reach_update waits, so the host clock round `--iters` calls is the time
of a build; one JSON line per combination of connectivity, THROUGH_UNKNOWN, clearance (min_d2 0 and 4) and budget (none
and 20 m) with the cells reached, the rounds, the tiles relaxed per round and the yardstick: the bytes one pass over the
result array moves (what k_frontier_classify does in 24.6 us).  Then 65,536 goal queries and 1,024 paths on the device,
and, in the same run, what the build replaces: voxels() plus tests/reach_ref.py on the same map, bounded by a budget so
that it finishes (--host-ref).  SDM_REACH_BATCH=k in the environment changes how many rounds are issued between two
looks at the count of active tiles (--batches runs the first combination under several).  Kernel times come from a
separate run, without counters, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/reach_probe.py --iters 3`.

  python tools/probes/reach_probe.py [--iters N] [--frames F] [--host-ref] [--host-ref-cost C] [--batches]
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


def build_us(m, iters, **kw):
    m.reach_update(**kw)
    t0 = time.perf_counter()
    for _ in range(iters):
        m.reach_update(**kw)
    return (time.perf_counter() - t0) / iters * 1e6


def start_cell(trav, word, reach=32):
    """the traversable cell nearest to cell `word` (looked for `reach` cells round it, then anywhere) and its distance in cells"""
    NZ, NY, NX = trav.shape
    c0 = np.array([word % NX, (word // NX) % NY, word // (NX * NY)])
    lo = np.maximum(c0 - reach, 0)
    cells = np.argwhere(trav[lo[2]:c0[2] + reach + 1, lo[1]:c0[1] + reach + 1, lo[0]:c0[0] + reach + 1])[:, ::-1] + lo
    if not len(cells):
        cells = np.argwhere(trav)[:, ::-1]
    d2 = ((cells - c0) ** 2).sum(axis=1)
    near = cells[np.argmin(d2)]
    return int(near[0] + NX * (near[1] + NY * near[2])), float(np.sqrt(d2.min()))


def report(tag, m, iters, start, moved=0.0, **kw):
    us = build_us(m, iters, start_cells=[start], **kw)
    _, info, _ = m.reach()
    rounds = int(info["rounds"])
    V = m.V
    print(json.dumps(dict({"reach": tag, "voxels": V, "us_per_build": round(us, 1), "rounds": rounds,
                           "tiles_per_round": round(m.reach_tiles() / max(rounds, 1), 1), "us_per_round": round(us / max(rounds, 1), 2),
                           "n_starts_used": int(info["n_starts_used"]), "n_traversable": int(info["n_traversable"]),
                           "n_reached": int(info["n_reached"]), "max_cost_reached": int(info["max_cost_reached"]),
                           "one_pass_bytes": V * 8 + V * 4 + V // 8, "one_pass_us_at_6TBps": round((V * 8 + V * 4 + V // 8) / 6e12 * 1e6, 2),
                           "start_moved_cells": round(moved, 1), "batch": os.environ.get("SDM_REACH_BATCH", "default"), "iters": iters},
                          **{k: (int(v) if not isinstance(v, bool) else v) for k, v in kw.items()})), flush=True)
    return info


def timed_device(m, fn, iters=10):
    for _ in range(2):
        fn()
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    m.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--host-ref", action="store_true")
    ap.add_argument("--host-ref-cost", type=int, default=300)
    ap.add_argument("--batches", action="store_true")
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
    m.esdf_update()
    m.synchronize()
    from tests import query_ref as qr
    from tests import reach_ref as rr
    geo = qr.Geometry(cfg, m.ring_state())
    cam = np.array([m.ring_state()["last_pos"]], np.float32)
    cam_word = int(rr.words_of_points(geo, cam)[0])
    occ, d2 = rr.occ_grid(geo, m.voxels()), m.esdf()[0]   # (the field is this frame's: one grid serves both rules)
    starts = {(through, min_d2): start_cell(rr.traversable(occ, through) & (d2 >= min_d2), cam_word) for through in (False, True) for min_d2 in (0, 4)}
    budget_20m = int(20.0 / (cfg["voxel_size"] * 0.1))
    if args.batches:
        for b in (1, 2, 4, 8, 16, 32):
            os.environ["SDM_REACH_BATCH"] = str(b)
            report("batch_C3", m, args.iters, *starts[True, 0], through_unknown=True)
        os.environ.pop("SDM_REACH_BATCH")
    for through in (False, True):
        for face in (False, True):
            for min_d2 in (0, 4):
                for max_cost in (0, budget_20m):
                    report("update_C3", m, args.iters, *starts[through, min_d2], face_connected=face, through_unknown=through, min_d2=min_d2,
                           max_cost=max_cost)
    # goals on the device: 65,536 queries, 1,024 paths of up to 256 cells, on the field through the unknown without a budget
    start = [starts[True, 0][0]]
    m.reach_update(start_cells=start, through_unknown=True)
    _, info, origin = m.reach()
    rng = np.random.default_rng(1)
    size = cfg["voxel_size"]
    pts = (origin + rng.uniform(0, 256 * size, (65536, 3))).astype(np.float32)
    d_pts, d_out = m.device_put(pts), m.device_alloc(65536 * 16)
    us_q = timed_device(m, lambda: m.query_reach(xyz=d_pts, n=65536, out=d_out, on_device=True))
    res = m.device_download(d_out, 65536 * 16, binding.REACH_RESULT)
    d_rows, d_lens = m.device_alloc(1024 * 256 * 4), m.device_alloc(1024 * 4)
    us_p = timed_device(m, lambda: m.reach_paths(xyz=d_pts, n=1024, max_len=256, on_device=True, cells_out=d_rows, len_out=d_lens))
    lens = m.device_download(d_lens, 1024 * 4, np.int32)
    print(json.dumps({"reach": "goals_C3", "queries": 65536, "us_per_query_call": round(us_q, 1), "reached": int((res["status"] == 0).sum()),
                      "paths": 1024, "us_per_paths_call": round(us_p, 1), "mean_path_cells": round(float(lens.mean()), 1),
                      "longest_path_cells": int(lens.max()), "us_per_step_of_the_longest": round(us_p / max(int(lens.max()), 1), 2)}), flush=True)
    if args.host_ref:
        for through in (False, True):
            kw = dict(through_unknown=through, max_cost=args.host_ref_cost)
            t0 = time.perf_counter()
            vox = m.voxels()
            t1 = time.perf_counter()
            start = [starts[through, 0][0]]
            ref = rr.field_of_map(geo, vox, start, **kw)
            t2 = time.perf_counter()
            us = build_us(m, args.iters, start_cells=start, **kw)
            cost, info, _ = m.reach()
            print(json.dumps({"reach": "host_replacement_C3", "through_unknown": through, "max_cost": args.host_ref_cost,
                              "download_ms": round((t1 - t0) * 1e3, 1), "python_ms": round((t2 - t1) * 1e3, 1), "device_us": round(us, 1),
                              "n_reached": int(info["n_reached"]), "equal": rr.equal_all(cost, info, ref) is None}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
