"""Times view scoring (sdm_query_views) on the C3 map (256^3), prefilled to ~2 M particles (synth.prefill_state) plus a few
frames of the street scene: 256 views at the centroids of the frontier clusters and at random free cells, random yaw, the
rays of every 8th pixel of the map's own camera (binding.pinhole_rays), range 10 m, device mode.  Host clock around
`--iters` back-to-back calls ended by one sdm_synchronize, after warm-up; one JSON line per variant: gains only and with
the per-ray outputs, under both ways of clearing the masks (SDM_VIEW_CLEAR=memset / rewalk), and with the views in flight
bounded to 1, 8 and the pool's size.  Yardstick 1, in the same run: the same n_views * n_rays segments, built on the host,
through sdm_query_segments - the walk without distinctness.  Yardstick 2 (--host-ref N): voxels() plus
tests/views_ref.py on the first N views (the NumPy walk takes seconds per view; the line says what N was).  Kernel times
come from a separate run, without counters, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/views_probe.py --iters 20`

(once with `--only memset`, once with `--only rewalk`: the calls of one clearing scheme, the pool's batches, gains only).

  python tools/probes/views_probe.py [--iters N] [--frames F] [--views V] [--stride S] [--range R] [--host-ref N] [--only memset|rewalk]
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


def candidate_views(m, cfg, n, rng_m, seed):
    """n views: the centroids of the largest frontier clusters (at most half of them), then random free cells"""
    from tests import frontiers_ref as fr
    from tests import query_ref as qr
    rng = np.random.default_rng(seed)
    m.frontiers_update(min_cells=8)
    table, origin = m.frontiers()
    order = np.argsort(-table["n_cells"].astype(np.int64), kind="stable")[:n // 2]
    pos = [table["centroid"][i] for i in order]
    geo = qr.Geometry(cfg, m.ring_state())
    occ = fr.occ_grid(geo, m.voxels())
    z, y, x = np.nonzero(occ == 0)
    pick = rng.choice(len(x), n - len(pos), replace=False)
    size = np.float32(cfg["voxel_size"])
    for i in pick:
        pos.append(origin + (np.array([x[i], y[i], z[i]], np.float32) + np.float32(0.5)) * size)
    views = np.zeros(n, binding.VIEW)
    views["pos"] = np.array(pos, np.float32)
    views["q"] = np.array([synth.yaw_quat(a) for a in rng.uniform(-np.pi, np.pi, n)], np.float32)
    views["range"] = rng_m
    return views, len(order)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--host-ref", type=int, default=0)
    ap.add_argument("--only", choices=("memset", "rewalk"), default=None, help="one way of clearing, the pool's batches, gains only (for a kernel trace)")
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
    views, n_frontier = candidate_views(m, cfg, args.views, args.range, 3)
    dirs = np.ascontiguousarray(binding.pinhole_rays(cfg, args.stride).reshape(-1, 3))
    nv, nr = len(views), len(dirs)
    d_views, d_dirs = m.device_put(views), m.device_put(dirs)
    d_out, d_rays, d_unk = m.device_alloc(nv * 40), m.device_alloc(nv * nr * 16), m.device_alloc(nv * nr * 4)
    base = dict(voxels=m.V, views=nv, views_at_frontiers=n_frontier, rays_per_view=nr, range_m=args.range, iters=args.iters,
                prefill_particles=int(n_pre))

    def call(with_rays):
        m.query_views(d_views, d_dirs, on_device=True, n_views=nv, n_rays=nr, out=d_out, rays_out=d_rays if with_rays else None,
                      ray_unknown_out=d_unk if with_rays else None)

    call(False)
    m.synchronize()
    gain = m.device_download(d_out, nv * 40).view(binding.VIEW_GAIN)
    marked = int(gain["n_unknown"].sum() + gain["n_free"].sum() + gain["n_occupied"].sum())
    base.update(marked_cells=marked, ray_cells=int(gain["ray_cells"].sum()), ray_unknown=int(gain["ray_unknown"].sum()),
                distinct_unknown=int(gain["n_unknown"].sum()), rays_hit=int(gain["rays_hit"].sum()), rays_in_map=int(gain["rays_in_map"].sum()),
                best_view_unknown=int(gain["n_unknown"].max()), median_view_unknown=int(np.median(gain["n_unknown"])))
    for clear in ("memset", "rewalk") if args.only is None else (args.only,):
        os.environ["SDM_VIEW_CLEAR"] = clear
        for batch in (0, 8, 1) if args.only is None else (0,):
            m.set_view_batch(batch)
            for with_rays in (False, True):
                if (batch or args.only) and with_rays:
                    continue
                us = timed(m, lambda: call(with_rays), args.iters)
                print(json.dumps(dict(base, views_probe="query_views", clear=clear, views_in_flight=batch or "pool", per_ray_outputs=with_rays,
                                      us_per_call=round(us, 1), ns_per_ray_cell=round(us * 1e3 / max(base["ray_cells"], 1), 3))), flush=True)
        m.set_view_batch(0)
        m.synchronize()
        assert m.device_download(d_out, nv * 40).tobytes() == gain.tobytes(), clear
    del os.environ["SDM_VIEW_CLEAR"]
    # yardstick 1: the same segments through sdm_query_segments (no distinctness, the rays built on the host)
    from tests import views_ref as vr
    a, b, _ = vr.rays_of(views, dirs)
    ab = np.ascontiguousarray(np.concatenate([a.reshape(-1, 3), b.reshape(-1, 3)], axis=1))
    d_ab = m.device_put(ab)
    us_seg = timed(m, lambda: m.query_segments(d_ab, on_device=True, n=nv * nr, out=d_rays), args.iters)
    seg = m.device_download(d_rays, nv * nr * 16).view(binding.SEGMENT_HIT)
    call(True)
    m.synchronize()
    same = m.device_download(d_rays, nv * nr * 16).tobytes() == seg.tobytes()
    print(json.dumps(dict(base, views_probe="query_segments_same_rays", us_per_call=round(us_seg, 1), rays_equal_bit_for_bit=same,
                          ns_per_ray_cell=round(us_seg * 1e3 / max(base["ray_cells"], 1), 3))), flush=True)
    if args.host_ref > 0:
        from tests import query_ref as qr
        k = min(args.host_ref, nv)
        t0 = time.perf_counter()
        vox = m.voxels()
        t1 = time.perf_counter()
        ref, _, _ = vr.query_views(qr.Geometry(cfg, m.ring_state()), vox, views[:k], dirs)
        t2 = time.perf_counter()
        # (a pinhole table has ambiguous rays - the optical axis runs along a lattice line from a cell centre -: counted, not asserted)
        differ = int(sum((ref[f] != gain[:k][f]).sum() for f in binding.VIEW_GAIN.names))
        print(json.dumps({"views_probe": "host_replacement_C3", "download_ms": round((t1 - t0) * 1e3, 1), "views_walked": k,
                          "numpy_ms_per_view": round((t2 - t1) * 1e3 / k, 1), "fields_differing": differ}), flush=True)
    for ptr in (d_views, d_dirs, d_out, d_rays, d_unk, d_ab):
        m.device_free(ptr)
    m.close()


if __name__ == "__main__":
    main()
