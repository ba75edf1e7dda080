"""Times the world archive's export, import and retain on the C3 archive of tools/probes/world_probe.py (256^3, prefilled to
~2 M particles plus a few frames of the street scene, one sdm_world_update).  Every time is taken with HIP events recorded
on the map's stream around the calls, averaged over `--iters` runs:
  * the export: sdm_get_world_bricks of the whole archive (host mode: the gather, the copy to the host, the wait);
  * sdm_world_import of that export into an empty archive at offset 0 and at offset (1, 2, 3), device mode (the sources
    are uploaded once, outside the window; each run is preceded by sdm_world_clear, outside the window);
  * a FILL import of the export onto itself, device mode: every brick is archived, no cell writes;
  * sdm_world_retain that keeps the lower half in z (each run preceded by clear + import, outside the window; the call
    waits, so its window ends after its own wait);
and, in the same process, as yardsticks: sdm_world_update in the steady state, and one device-to-device copy of the same
brick bytes (2048 B of words and 20 B of header per brick).  One JSON line each, with the bytes the call has to move (the
least: what it reads of the sources and of the pool and what it writes; hash probes, candidate arrays, scans and sorts not
counted) and that figure over the copy's time.  The lines also go to profiles/world_io_probe.txt (--out).

  python tools/probes/world_io_probe.py [--iters N] [--frames F] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_dsp_map_amd import binding, synth  # noqa: E402
from tools.probes.world_probe import HIP, Events, hip  # noqa: E402

BRICK = 2048 + 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_io_probe.txt"))
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
        text = json.dumps(dict({"world_io": "C3", "what": what, "us": round(us, 1)}, **kw))
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    m.world_update()
    hdr, cells = m.world_bricks()
    n = len(hdr)
    known = int((cells >> 24 != 0xFF).sum())
    d_hdr, d_cells, d_copy = m.device_put(hdr), m.device_put(cells), m.device_alloc(n * BRICK)
    imp = lambda **kw: m.world_import(d_hdr, d_cells, on_device=True, n=n, **kw)  # noqa: E731

    # the yardsticks
    us_update = ev.time_us(m.world_update, args.iters)
    copy = lambda: (hip(HIP.hipMemcpyAsync(C.c_void_p(d_copy), C.c_void_p(d_cells), C.c_size_t(n * 2048), 3, C.c_void_p(m.stream()))),  # noqa: E731
                    hip(HIP.hipMemcpyAsync(C.c_void_p(d_copy + n * 2048), C.c_void_p(d_hdr), C.c_size_t(n * 20), 3, C.c_void_p(m.stream()))))
    copy()
    us_copy = ev.time_us(copy, args.iters)
    line("yardstick_world_update_steady", us_update, n_bricks=n)
    line("yardstick_copy_d2d", us_copy, bytes=n * BRICK, TBps=round(2 * n * BRICK / us_copy / 1e6, 3))

    def report(what, us, moved, **kw):
        line(what, us, n_bricks=n, known_cells=known, bytes_moved=moved, TBps=round(moved / us / 1e6, 3),
             times_the_copy=round(us / us_copy, 2), **kw)

    # the export: pool -> staging (read + write), staging -> host
    us = ev.time_us(lambda: m.world_bricks(), args.iters)
    report("export_host", us, 3 * n * BRICK)
    # into an empty archive: the sources are read twice (mark, merge), every destination is written whole
    for offset, fan in (((0, 0, 0), 1), ((1, 2, 3), 8)):
        imp(offset=offset)                                   # warm-up: the work arrays
        us = ev.time_us(lambda: imp(offset=offset), args.iters, before=m.world_clear)
        info = m.world_info()
        created = int(info["created_last"])
        report("import_empty_offset_%d_%d_%d" % offset, us, 2 * n * BRICK + created * BRICK, created=created, dropped=int(info["dropped_last"]),
               pairs=n * fan)
    # FILL onto itself: sources read once and the pool once (mark); nothing writes, so merge returns at once
    m.world_clear()
    imp()
    us = ev.time_us(lambda: imp(fill=True), args.iters)
    info = m.world_info()
    report("import_fill_onto_itself", us, 2 * n * 2048 + n * 20, created=int(info["created_last"]))
    # retain the lower half in z: kept bricks go to the transient copy and back (2 reads, 2 writes), the table is rebuilt
    half = int(np.sort(hdr["bz"])[n // 2])
    removed = []

    def refill():
        m.world_clear()
        imp()

    us = ev.time_us(lambda: removed.append(m.world_retain(bmax=(32767, 32767, half - 1))), args.iters, before=refill)
    kept = n - removed[-1]
    report("retain_lower_half", us, 4 * kept * BRICK + n * 20, kept=kept, removed=removed[-1])
    for p in (d_hdr, d_cells, d_copy):
        m.device_free(p)
    m.close()
    out.close()


if __name__ == "__main__":
    main()
