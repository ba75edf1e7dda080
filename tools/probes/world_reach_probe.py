"""Times world reach on the archive of the C3 map (256^3; tools/probes/world_probe.py's: prefilled to ~2 M particles plus a
few frames of the street scene, one sdm_world_update), the start at the camera:
  * sdm_world_reach_update, which waits, in host microseconds per build (the median of `--iters`), with the rounds it took
    and the bricks it relaxed per round: both connectivities, inflate 0 and 1, without and with a budget of 20 m;
  * sdm_query_world_reach for 65,536 goals and sdm_world_reach_paths for 1,024, device mode, between HIP events;
and, in the same process, the yardsticks: sdm_reach_update on the block from the same start (host microseconds, it
waits too) and the steady sdm_world_update (HIP events).  Cells that were never observed can be crossed in both fields
(THROUGH_UNKNOWN), so that the two builds cover the same cells.  One JSON line each.

  python tools/probes/world_reach_probe.py [--iters N] [--frames F]
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
from tools.probes.world_probe import Events  # noqa: E402


def host_us(fn, iters):
    times = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e6)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    args = ap.parse_args()
    cfg, params = synth.CONFIGS["C3"], synth.PARAMS["vkitti2"]
    scene = synth.Scene(cfg, n_static=48, n_dynamic=6, seed=7)
    st, ring, n_pre = synth.prefill_state(cfg, scene, 2000000)
    m = binding.SdmMap(cfg, params, synth.noise_table())
    m.load_state(st)
    m.set_ring_state(ring)
    pos = q = None
    for t in range(args.frames):
        depth, cloud, pos, q = scene.render(t, params)
        m.update(depth, cloud, pos, q, scene.moves(t))
    m.synchronize()
    size = float(cfg["voxel_size"])
    m.world_update()
    winfo = m.world_info()
    start = np.asarray(pos, np.float32).reshape(1, 3)

    def line(what, us, **kw):
        print(json.dumps(dict({"world": "C3", "what": what, "us": round(us, 1)}, **kw)), flush=True)

    budget = int(round(20.0 / (size * 0.1)))
    m.world_reach_update(starts=start, through_unknown=True)   # warm-up: code objects, the buffers
    for face in (False, True):
        for inflate in (0, 1):
            for max_cost in (0, budget):
                build = lambda: m.world_reach_update(starts=start, inflate=inflate, max_cost=max_cost, face_connected=face, through_unknown=True)  # noqa: E731
                us = host_us(build, args.iters)
                info = m.world_reach(with_cost=False)[2]
                relaxed = m.world_reach_bricks_relaxed()
                line("world_reach_update", us, face_connected=face, inflate=inflate, max_cost=max_cost, n_bricks=int(info["n_bricks"]),
                     n_starts_used=int(info["n_starts_used"]), n_traversable=int(info["n_traversable"]), n_reached=int(info["n_reached"]),
                     max_cost_reached=int(info["max_cost_reached"]), rounds=int(info["rounds"]), bricks_relaxed=relaxed,
                     bricks_per_round=round(relaxed / max(int(info["rounds"]), 1), 1), us_per_round=round(us / max(int(info["rounds"]), 1), 1))
    # the queries, device mode, on the 26-connected field without budget
    m.world_reach_update(starts=start, through_unknown=True)
    ev = Events(m.stream())
    rng = np.random.default_rng(5)
    lo, hi = winfo["bmin"].astype(np.float64) * 8, (winfo["bmax"].astype(np.float64) + 1) * 8
    n, n_paths, max_len = 65536, 1024, 1024
    xyz = ((rng.uniform(lo, hi, (n, 3)).astype(np.int64).astype(np.float32) + np.float32(0.5)) * np.float32(size)).astype(np.float32)
    d_xyz, d_out = m.device_put(xyz), m.device_alloc(n * 24)
    d_rows, d_lens = m.device_alloc(n_paths * max_len * 12), m.device_alloc(n_paths * 4)
    query = lambda: m.query_world_reach(xyz=d_xyz, on_device=True, n=n, out=d_out)  # noqa: E731
    query()
    us = ev.time_us(query, args.iters)
    res = m.device_download(d_out, n * 24, binding.WORLD_REACH_RESULT)
    line("query_world_reach_64K", us, goals=n, reached=int((res["status"] == 0).sum()), Mgoals_per_s=round(n / us, 1))
    paths = lambda: m.world_reach_paths(xyz=d_xyz, max_len=max_len, on_device=True, n=n_paths, cells_out=d_rows, len_out=d_lens)  # noqa: E731
    paths()
    us = ev.time_us(paths, args.iters)
    lens = m.device_download(d_lens, n_paths * 4, np.int32)
    line("world_reach_paths_1K", us, goals=n_paths, with_path=int((lens > 0).sum()), mean_len=round(float(lens[lens > 0].mean()) if (lens > 0).any() else 0.0, 1),
         longest=int(lens.max()), us_per_step=round(us / max(int(lens.max()), 1), 2))
    # the yardsticks
    for face in (False, True):
        for max_cost in (0, budget):
            build = lambda: m.reach_update(starts=start, max_cost=max_cost, face_connected=face, through_unknown=True)  # noqa: E731
            build()
            us = host_us(build, args.iters)
            info = m.reach()[1]
            line("yardstick_reach_update", us, face_connected=face, max_cost=max_cost, n_traversable=int(info["n_traversable"]),
                 n_reached=int(info["n_reached"]), max_cost_reached=int(info["max_cost_reached"]), rounds=int(info["rounds"]),
                 tiles_relaxed=m.reach_tiles(), us_per_round=round(us / max(int(info["rounds"]), 1), 1))
    m.world_update()
    m.synchronize()
    us = ev.time_us(m.world_update, args.iters)
    line("yardstick_steady_world_update", us, n_bricks=int(m.world_info()["n_bricks"]))
    for p in (d_xyz, d_out, d_rows, d_lens):
        m.device_free(p)
    m.close()


if __name__ == "__main__":
    main()
