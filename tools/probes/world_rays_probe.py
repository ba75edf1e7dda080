"""Times world rays on the archive of the C3 map (256^3; tools/probes/world_probe.py's: prefilled to ~2 M particles plus a
few frames of the street scene, one sdm_world_update), medians of `--iters` between HIP events, device mode:
  * sdm_query_world_segments for 65,536 segments of about 100 cells, beside the block's sdm_query_segments on the same
    end points;
  * sdm_query_world_views for 32 views x 4,096 rays at reach_cells 64 and 128 (the range is the reach), beside
    sdm_query_views on the same poses.
One JSON line each, with the ratio to the block's call.  Every step runs under a time limit of its own: a step that exceeds
it ends the process (SIGALRM's default action), and the line printed before it says which step it was.  Where the time
goes - the walk kernel or the memset that clears the masks - comes from a separate run without counters, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/world_rays_probe.py --only views128` (or
segments, views64).

  python tools/probes/world_rays_probe.py [--iters N] [--frames F] [--only segments|views64|views128]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_dsp_map_amd import binding, synth  # noqa: E402
from tools.probes.world_esdf_probe import step  # noqa: E402
from tools.probes.world_probe import Events  # noqa: E402

N_SEGMENTS, SEGMENT_CELLS = 65536, 100
N_VIEWS, RAYS_SIDE = 32, 64


def median_us(ev, fn, iters):
    fn()
    return float(np.median([ev.time_us(fn, 1) for _ in range(iters)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--only", choices=("segments", "views64", "views128"), help="this call alone, no yardstick: for a kernel trace")
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
    size = np.float32(cfg["voxel_size"])
    ev = Events(m.stream())
    rng = np.random.default_rng(5)
    lo, hi = winfo["bmin"].astype(np.float64) * 8, (winfo["bmax"].astype(np.float64) + 1) * 8

    def line(what, us, **kw):
        print(json.dumps(dict({"world": "C3", "what": what, "us": round(us, 1), "n_bricks": int(winfo["n_bricks"])}, **kw)), flush=True)

    if args.only in (None, "segments"):
        with step("segments", 120):
            a = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), (N_SEGMENTS, 3))
            d = rng.standard_normal((N_SEGMENTS, 3))
            d *= (SEGMENT_CELLS - 1) / np.abs(d).sum(axis=1, keepdims=True)          # 1 + sum |d| cells
            ab = np.concatenate([a, a + d], axis=1).astype(np.float32) * size
            d_ab, d_out, d_blk = m.device_put(ab), m.device_alloc(N_SEGMENTS * 32), m.device_alloc(N_SEGMENTS * 16)
            world = lambda: m.query_world_segments(d_ab, on_device=True, n=N_SEGMENTS, out=d_out)  # noqa: E731
            us = median_us(ev, world, args.iters)
            res = m.device_download(d_out, N_SEGMENTS * 32, binding.WORLD_SEGMENT_HIT)
            walked = int(res["cells"].sum())
            kw = dict(segments=N_SEGMENTS, hits=int((res["t"] >= 0).sum()), cells_walked=walked, ns_per_cell=round(1e3 * us / max(walked, 1), 3))
            if args.only is None:
                block = lambda: m.query_segments(d_ab, on_device=True, n=N_SEGMENTS, out=d_blk)  # noqa: E731
                us_b = median_us(ev, block, args.iters)
                blk = m.device_download(d_blk, N_SEGMENTS * 16, binding.SEGMENT_HIT)
                kw.update(block_us=round(us_b, 1), block_cells_walked=int(blk["cells"].sum()), world_over_block=round(us / us_b, 2))
            line("query_world_segments_64K", us, **kw)
            for p in (d_ab, d_out, d_blk):
                m.device_free(p)
    x = ((np.arange(RAYS_SIDE, dtype=np.float32) + np.float32(0.5)) / np.float32(RAYS_SIDE) - np.float32(0.5)) * np.float32(1.6)
    dirs = np.empty((RAYS_SIDE, RAYS_SIDE, 3), np.float32)
    dirs[..., 0], dirs[..., 1], dirs[..., 2] = x[None, :], x[:, None], 1.0
    n_rays = RAYS_SIDE * RAYS_SIDE
    views = np.zeros(N_VIEWS, binding.VIEW)
    views["pos"] = (rng.uniform(lo + 0.3 * (hi - lo), hi - 0.3 * (hi - lo), (N_VIEWS, 3)) * size).astype(np.float32)
    yaw = rng.uniform(0, 2 * np.pi, N_VIEWS)
    views["q"] = np.stack([np.cos(yaw / 2), np.zeros(N_VIEWS), np.sin(yaw / 2), np.zeros(N_VIEWS)], 1).astype(np.float32)
    for reach in (64, 128):
        if args.only not in (None, "views%d" % reach):
            continue
        with step("views, reach %d" % reach, 120):
            views["range"] = np.float32(reach) * size
            d_v, d_d, d_g = m.device_put(views), m.device_put(dirs.reshape(-1, 3)), m.device_alloc(N_VIEWS * 40)
            world = lambda: m.query_world_views(d_v, d_d, reach, on_device=True, n_views=N_VIEWS, n_rays=n_rays, out=d_g)  # noqa: E731
            us = median_us(ev, world, args.iters)
            gain = m.device_download(d_g, N_VIEWS * 40, binding.VIEW_GAIN)
            walked = int(gain["ray_cells"].sum())
            kw = dict(views=N_VIEWS, rays=n_rays, reach_cells=reach, mask_MB=round((2 * reach + 1) ** 3 / 8e6, 2), cells_walked=walked,
                      distinct=int(gain["n_unknown"].sum() + gain["n_free"].sum() + gain["n_occupied"].sum()), ns_per_cell=round(1e3 * us / max(walked, 1), 3))
            if args.only is None:
                block = lambda: m.query_views(d_v, d_d, on_device=True, n_views=N_VIEWS, n_rays=n_rays, out=d_g)  # noqa: E731
                us_b = median_us(ev, block, args.iters)
                blk = m.device_download(d_g, N_VIEWS * 40, binding.VIEW_GAIN)
                kw.update(block_us=round(us_b, 1), block_cells_walked=int(blk["ray_cells"].sum()), world_over_block=round(us / us_b, 2))
            line("query_world_views_32x4096", us, **kw)
            for p in (d_v, d_d, d_g):
                m.device_free(p)
    m.close()


if __name__ == "__main__":
    main()
