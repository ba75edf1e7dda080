"""Times the world distance field on the archive of the C3 map (256^3; tools/probes/world_probe.py's: prefilled to ~2 M
particles plus a few frames of the street scene, one sdm_world_update):
  * sdm_world_esdf_update followed by a wait, at R = 4, 8, 9 and 16 - 27 neighbour bricks up to 8, 125 beyond - in host
    microseconds per build (the median of `--iters`), with the bricks, obstacle cells and cells within the radius it found
    and the microseconds per cell covered;
  * sdm_query_world_distance for 65,536 points, device mode, between HIP events;
and, in the same process, the yardsticks: sdm_esdf_update on the block followed by a wait (host microseconds, with its
microseconds per cell and the ratio of the two), and the steady sdm_world_update (HIP events).  One JSON line each.  Every
step runs under a time limit of its own: a step that exceeds it ends the process (SIGALRM's default action, which no call
into the library can hold up), and the line printed before it says which step it was.  Kernel times come from separate
runs, without counters, one radius each so that every k_we_* launch of the trace belongs to it, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/world_esdf_probe.py --only 16` (or 4, 8, 9).

  python tools/probes/world_esdf_probe.py [--iters N] [--frames F] [--only R]
"""
import argparse
import contextlib
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_dsp_map_amd import binding, synth  # noqa: E402
from tools.probes.world_probe import Events  # noqa: E402

RADII = (4, 8, 9, 16)


@contextlib.contextmanager
def step(name, seconds):
    print(json.dumps({"step": name, "limit_s": seconds}), flush=True)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


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
    ap.add_argument("--only", type=int, choices=RADII, help="builds of this radius alone, no warm-up of another, no query, no yardstick")
    args = ap.parse_args()
    cfg, params = synth.CONFIGS["C3"], synth.PARAMS["vkitti2"]
    with step("the C3 map and its archive", 240):
        scene = synth.Scene(cfg, n_static=48, n_dynamic=6, seed=7)
        st, ring, n_pre = synth.prefill_state(cfg, scene, 2000000)
        m = binding.SdmMap(cfg, params, synth.noise_table())
        m.load_state(st)
        m.set_ring_state(ring)
        for t in range(args.frames):
            depth, cloud, pos, q = scene.render(t, params)
            m.update(depth, cloud, pos, q, scene.moves(t))
        m.synchronize()
        m.world_update()
        m.synchronize()
        winfo = m.world_info()
    size = float(cfg["voxel_size"])

    def line(what, us, **kw):
        print(json.dumps(dict({"world": "C3", "what": what, "us": round(us, 1)}, **kw)), flush=True)

    def build_of(radius):
        def build():
            m.world_esdf_update(radius)
            m.synchronize()
        return build

    if args.only:
        with step("world_esdf_update R=%d alone" % args.only, 60):
            us = host_us(build_of(args.only), args.iters + 1)
            info = m.world_esdf(cap=0)[3]
            line("world_esdf_update", us, radius=args.only, builds=args.iters + 1, n_bricks=int(info["n_bricks"]))
        m.close()
        return
    with step("warm-up", 60):
        build_of(4)()        # code objects, the buffers
        build_of(16)()
        m.esdf_update()
        m.synchronize()
    world_us = {}
    for radius in RADII:
        with step("world_esdf_update R=%d" % radius, 60):
            us = host_us(build_of(radius), args.iters)
            info = m.world_esdf(cap=0)[3]
            cells = int(info["n_bricks"]) * 512
            world_us[radius] = us / max(cells, 1)
            line("world_esdf_update", us, radius=radius, neighbours=27 if radius <= 8 else 125, n_bricks=int(info["n_bricks"]),
                 n_obstacle_cells=int(info["n_obstacle_cells"]), n_near_cells=int(info["n_near_cells"]), ns_per_cell=round(1e3 * us / max(cells, 1), 3),
                 field_MB=round(cells * 4 / 1e6, 1), store_GB_per_s=round(cells * 4 / max(us, 1e-9) / 1e3, 1))
    line("step_8_to_9", 0.0, ratio=round(world_us[9] / world_us[8], 2), ratio_16_over_9=round(world_us[16] / world_us[9], 2))
    # the query, device mode, on the field of R = 16
    with step("query_world_distance 64K", 60):
        ev = Events(m.stream())
        rng = np.random.default_rng(5)
        lo, hi = winfo["bmin"].astype(np.float64) * 8, (winfo["bmax"].astype(np.float64) + 1) * 8
        n = 65536
        xyz = ((rng.uniform(lo, hi, (n, 3)).astype(np.int64).astype(np.float32) + np.float32(0.5)) * np.float32(size)).astype(np.float32)
        d_xyz, d_out = m.device_put(xyz), m.device_alloc(n * 32)
        query = lambda: m.query_world_distance(xyz=d_xyz, on_device=True, n=n, out=d_out)  # noqa: E731
        query()
        us = ev.time_us(query, args.iters)
        res = m.device_download(d_out, n * 32, binding.WORLD_DISTANCE_RESULT)
        line("query_world_distance_64K", us, points=n, in_field=int((res["d2"] != 0xFFFFFFFF).sum()), far=int((res["d2"] == binding.WORLD_ESDF_FAR).sum()),
             Mpoints_per_s=round(n / us, 1))
        m.device_free(d_xyz), m.device_free(d_out)
    # the yardsticks: the block's own exact field, and a steady archive update
    with step("yardstick esdf_update", 60):
        def block():
            m.esdf_update()
            m.synchronize()
        block()
        us = host_us(block, args.iters)
        per_cell = us / m.V
        line("yardstick_esdf_update", us, cells=int(m.V), ns_per_cell=round(1e3 * per_cell, 3),
             world_over_block_per_cell={str(r): round(world_us[r] / per_cell, 2) for r in RADII})
    with step("yardstick steady world_update", 60):
        m.world_update()
        m.synchronize()
        us = ev.time_us(m.world_update, args.iters)
        line("yardstick_steady_world_update", us, n_bricks=int(m.world_info()["n_bricks"]))
    m.close()


if __name__ == "__main__":
    main()
