"""Times the world ground layer on the archive of the C3 map (256^3; tools/probes/world_probe.py's: prefilled to ~2 M
particles plus a few frames of the street scene, one sdm_world_update):
  * sdm_world_ground_update followed by a wait, the up axis the scene's (1, -1), a band of 64 cells from the archive's
    lowest cell up, at R = 8 and R = 16 - 9 neighbour tiles up to 8, 25 beyond - in host microseconds per build (the median
    of `--iters`), with the tiles and the columns by class it found and the microseconds per archived brick and per tile;
  * sdm_query_world_ground for 65,536 points and sdm_query_world_footprints for 4,096 footprints of 1 m x 0.6 m, device
    mode, between HIP events;
and, in the same process on the same archive, the yardstick: sdm_world_esdf_update followed by a wait at the same radii (the
same bricks, three passes instead of two, 512 instead of 64 outputs per brick), with the ratio per archived brick.  One JSON
line each.  Every step runs under a time limit of its own (tools/probes/world_esdf_probe.py's `step`).  Kernel times come
from a separate run, without counters, one radius so that every k_wg_* launch of the trace belongs to it, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/world_ground_probe.py --only 16` (or 8).

  python tools/probes/world_ground_probe.py [--iters N] [--frames F] [--only R]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_dsp_map_amd import binding, synth  # noqa: E402
from tools.probes.world_esdf_probe import host_us, step  # noqa: E402
from tools.probes.world_probe import Events  # noqa: E402

RADII = (8, 16)
UP = (1, -1)
BAND = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
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
    n_arch = int(winfo["n_bricks"])
    # the lowest archived cell along the up axis, as a height
    g_max, g_min = (int(winfo["bmax"][UP[0]]) + 1) * 8 - 1, int(winfo["bmin"][UP[0]]) * 8
    h_lo = g_min if UP[1] > 0 else -1 - g_max
    opts = dict(up=UP, h_lo=h_lo, h_hi=h_lo + BAND - 1, clearance=4, max_step=1, support_labels=[synth.LABEL_ROAD])

    def line(what, us, **kw):
        print(json.dumps(dict({"world": "C3", "what": what, "us": round(us, 1)}, **kw)), flush=True)

    def build_of(radius):
        def build():
            m.world_ground_update(radius=radius, **opts)
            m.synchronize()
        return build

    def esdf_of(radius):
        def build():
            m.world_esdf_update(radius)
            m.synchronize()
        return build

    if args.only:
        with step("world_ground_update R=%d alone" % args.only, 60):
            us = host_us(build_of(args.only), args.iters + 1)
            info = m.world_ground(cap=0)[3]
            line("world_ground_update", us, radius=args.only, builds=args.iters + 1, n_tiles=int(info["n_tiles"]), n_archived_bricks=n_arch)
        m.close()
        return
    with step("warm-up", 60):
        for radius in RADII:     # code objects, the buffers
            build_of(radius)()
            esdf_of(radius)()
    ground_us = {}
    for radius in RADII:
        with step("world_ground_update R=%d" % radius, 60):
            us = host_us(build_of(radius), args.iters)
            info = m.world_ground(cap=0)[3]
            tiles = int(info["n_tiles"])
            ground_us[radius] = us
            line("world_ground_update", us, radius=radius, neighbours=9 if radius <= 8 else 25, n_archived_bricks=n_arch, n_tiles=tiles, band=BAND,
                 h_lo=h_lo, n_ground=int(info["n_ground"]), n_obstacle=int(info["n_obstacle"]), n_none=int(info["n_none"]), n_step=int(info["n_step"]),
                 n_lethal=int(info["n_lethal"]), ns_per_archived_brick=round(1e3 * us / max(n_arch, 1), 1), ns_per_tile=round(1e3 * us / max(tiles, 1), 1))
    for radius in RADII:
        with step("yardstick world_esdf_update R=%d" % radius, 60):
            us = host_us(esdf_of(radius), args.iters)
            info = m.world_esdf(cap=0)[3]
            line("yardstick_world_esdf_update", us, radius=radius, n_bricks=int(info["n_bricks"]), ns_per_archived_brick=round(1e3 * us / max(n_arch, 1), 1),
                 esdf_over_ground=round(us / ground_us[radius], 2))
    # the queries, device mode, on the layer of R = 16
    with step("queries", 60):
        ev = Events(m.stream())
        rng = np.random.default_rng(5)
        lo, hi = winfo["bmin"].astype(np.float64) * 8, (winfo["bmax"].astype(np.float64) + 1) * 8
        n = 65536
        xyz = ((rng.uniform(lo, hi, (n, 3)).astype(np.int64).astype(np.float32) + np.float32(0.5)) * np.float32(size)).astype(np.float32)
        d_xyz, d_out = m.device_put(xyz), m.device_alloc(n * 40)
        query = lambda: m.query_world_ground(xyz=d_xyz, on_device=True, n=n, out=d_out)  # noqa: E731
        query()
        us = ev.time_us(query, args.iters)
        res = m.device_download(d_out, n * 40, binding.WORLD_GROUND_RESULT)
        line("query_world_ground_64K", us, points=n, in_tiles=int((res["status"] == 0).sum()), far=int((res["d2"] == binding.WORLD_GROUND_FAR).sum()),
             Mpoints_per_s=round(n / us, 1))
        m.device_free(d_xyz), m.device_free(d_out)
        k = 4096
        au, av = (1 if UP[0] == 0 else 0), (1 if UP[0] == 2 else 2)
        fps = np.zeros(k, binding.FOOTPRINT)
        t = rng.uniform(0, 2 * np.pi, k)
        fps["center_u"], fps["center_v"] = rng.uniform(lo[au], hi[au], k) * size, rng.uniform(lo[av], hi[av], k) * size
        fps["dir_u"], fps["dir_v"], fps["half_len"], fps["half_wid"] = np.cos(t), np.sin(t), 0.5, 0.3
        d_fp, d_out = m.device_put(fps), m.device_alloc(k * 40)
        query = lambda: m.query_world_footprints(d_fp, on_device=True, n=k, out=d_out)  # noqa: E731
        query()
        us = ev.time_us(query, args.iters)
        res = m.device_download(d_out, k * 40, binding.WORLD_FOOTPRINT_RESULT)
        line("query_world_footprints_4K", us, footprints=k, columns=int(res["n_cols"].sum()), absent=int(res["n_absent"].sum()),
             lethal=int((res["n_lethal"] > 0).sum()), Kfootprints_per_s=round(1e3 * k / us, 1))
        m.device_free(d_fp), m.device_free(d_out)
    m.close()


if __name__ == "__main__":
    main()
