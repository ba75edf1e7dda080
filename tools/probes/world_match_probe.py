"""Times sdm_world_match on the C3 archive of tools/probes/world_probe.py (256^3, prefilled to ~2 M particles plus a few
frames of the street scene, one sdm_world_update), with the whole archive as the source, device mode (the sources are
uploaded once, outside the window).  Every device time is taken with HIP events recorded on the map's stream around the
calls, averaged over `--iters` runs:
  * a match at the radii (0, 0, 0), (2, 2, 1), (4, 4, 2) and (8, 8, 8) round the offset (1, 2, 3), with and without the
    candidates' records (scores == NULL);
and, in the same process, as yardsticks: sdm_world_import of the same sources into an empty archive at offset 0 (device
mode, each run preceded by sdm_world_clear outside the window - it leaves the archive as it was), one device-to-device
copy of the same brick bytes, and the NumPy grid model of tests/world_match_ref.py at the two smallest radii (wall clock,
one run; --no-model skips it).  One JSON line each, with the cell pairs a match looks at (counted source cells x
candidates) and that figure per microsecond.  The lines also go to profiles/world_match_probe.txt (--out).

  python tools/probes/world_match_probe.py [--iters N] [--frames F] [--no-model] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_dsp_map_amd import binding, synth  # noqa: E402
from tools.probes.world_probe import HIP, Events, hip  # noqa: E402

BRICK = 2048 + 20
RADII = ((0, 0, 0), (2, 2, 1), (4, 4, 2), (8, 8, 8))
OFFSET = (1, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_match_probe.txt"))
    args = ap.parse_args()
    cfg, params = synth.CONFIGS["C3"], synth.PARAMS["vkitti2"]
    scene = synth.Scene(cfg, n_static=48, n_dynamic=6, seed=7)
    st, ring, _ = synth.prefill_state(cfg, scene, 2000000)
    m = binding.SdmMap(cfg, params, synth.noise_table())
    m.load_state(st)
    m.set_ring_state(ring)
    for t in range(args.frames):
        depth, cloud, pos, q = scene.render(t, params)
        m.update(depth, cloud, pos, q, scene.moves(t))
    m.synchronize()
    ev = Events(m.stream())
    out = open(args.out, "w")

    def line(what, us, **kw):
        text = json.dumps(dict({"world_match": "C3", "what": what, "us": round(us, 1)}, **kw))
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    m.world_update()
    hdr, cells = m.world_bricks()
    n = len(hdr)
    counted = int((cells >> 24 != 0xFF).sum())
    d_hdr, d_cells, d_copy = m.device_put(hdr), m.device_put(cells), m.device_alloc(n * BRICK)
    d_scores = m.device_alloc(17 ** 3 * binding.WORLD_MATCH_SCORE.itemsize)
    d_res = m.device_alloc(binding.WORLD_MATCH_RESULT.itemsize)

    # the yardsticks
    copy = lambda: (hip(HIP.hipMemcpyAsync(C.c_void_p(d_copy), C.c_void_p(d_cells), C.c_size_t(n * 2048), 3, C.c_void_p(m.stream()))),  # noqa: E731
                    hip(HIP.hipMemcpyAsync(C.c_void_p(d_copy + n * 2048), C.c_void_p(d_hdr), C.c_size_t(n * 20), 3, C.c_void_p(m.stream()))))
    copy()
    us_copy = ev.time_us(copy, args.iters)
    line("yardstick_copy_d2d", us_copy, n_bricks=n, bytes=n * BRICK)
    imp = lambda: m.world_import(d_hdr, d_cells, on_device=True, n=n)  # noqa: E731
    m.world_clear()
    imp()                                                    # warm-up: the work arrays
    us_import = ev.time_us(imp, args.iters, before=m.world_clear)
    line("yardstick_import_empty_offset_0", us_import, n_bricks=n, created=int(m.world_info()["created_last"]))

    for radius in RADII:
        cand = int(np.prod([2 * r + 1 for r in radius]))
        for with_scores in (True, False):
            match = lambda: m.world_match(d_hdr, d_cells, offset=OFFSET, radius=radius, on_device=True, n=n,  # noqa: E731
                                          scores=d_scores if with_scores else None, result=d_res)
            match()                                          # warm-up: the work arrays
            us = ev.time_us(match, args.iters)
            res = m.device_download(d_res, binding.WORLD_MATCH_RESULT.itemsize).view(binding.WORLD_MATCH_RESULT)[0]
            line("match_radius_%d_%d_%d%s" % (radius + ("" if with_scores else "_no_scores",)), us, n_bricks=n, candidates=cand, counted_cells=counted,
                 pairs=counted * cand, pairs_per_us=round(counted * cand / us, 1), times_the_import=round(us / us_import, 2),
                 times_the_copy=round(us / us_copy, 2), best_offset=[int(v) for v in res["best_offset"]], best_score=int(res["best_score"]),
                 runner_up=int(res["runner_up"]))

    if not args.no_model:
        from tests import world_match_ref as mr
        mm = cfg["max_movable_track"]
        for radius in RADII[:2]:
            t0 = time.perf_counter()
            want, _ = mr.dense(hdr, cells, hdr, cells, offset=OFFSET, radius=radius, max_movable=mm)
            us = (time.perf_counter() - t0) * 1e6
            got, _ = m.world_match(hdr, cells, offset=OFFSET, radius=radius)
            line("yardstick_numpy_grid_model_radius_%d_%d_%d" % radius, us, same_bytes=bool(want.tobytes() == got.tobytes()))
    for p in (d_hdr, d_cells, d_copy, d_scores, d_res):
        m.device_free(p)
    m.close()
    out.close()


if __name__ == "__main__":
    main()
