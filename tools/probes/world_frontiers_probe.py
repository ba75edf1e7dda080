"""Times the world frontiers on the archive of the C3 map (256^3; tools/probes/world_probe.py's: prefilled to ~2 M particles
plus a few frames of the street scene, one sdm_world_update), under 26- and 6-connectivity:
  * sdm_world_frontiers_update, which waits, in host microseconds per build (the median of `--iters`), with the bricks,
    cells and clusters it found, without and with INSIDE_BRICKS;
and, in the same process, the yardstick: sdm_frontiers_update on the block that holds the same cells, ended by a
sdm_synchronize (host microseconds, the median of `--iters`), and the ratio of the two.  One JSON line each.  Every step
runs under a time limit of its own: a step that exceeds it ends the process (SIGALRM's default action, which no call into
the library can hold up), and the line printed before it says which step it was.  Kernel times come from separate runs,
without counters, one connectivity each so that every k_wf_* launch of the trace belongs to it, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/world_frontiers_probe.py --only 26` (or 6).

  python tools/probes/world_frontiers_probe.py [--iters N] [--frames F] [--only 26|6]
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
    ap.add_argument("--only", choices=("26", "6"), help="builds of this connectivity alone (absent bricks unknown), no warm-up of the other, no yardstick")
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

    def line(what, us, **kw):
        print(json.dumps(dict({"world": "C3", "what": what, "us": round(us, 1)}, **kw)), flush=True)

    if args.only:
        face = args.only == "6"
        with step("world_frontiers_update face=%s alone" % face, 60):
            us = host_us(lambda: m.world_frontiers_update(face_connected=face), args.iters + 1)
            info = m.world_frontiers()[1]
            line("world_frontiers_update", us, face_connected=face, inside_bricks=False, builds=args.iters + 1, n_cells=int(info["n_cells"]))
        m.close()
        return
    with step("warm-up", 60):
        m.world_frontiers_update()   # code objects, the buffers
        m.frontiers_update()
        m.synchronize()
    world_us = {}
    for face in (False, True):
        for inside in (False, True):
            with step("world_frontiers_update face=%s inside=%s" % (face, inside), 60):
                us = host_us(lambda: m.world_frontiers_update(face_connected=face, inside_bricks=inside), args.iters)
                table, info = m.world_frontiers()
                world_us[(face, inside)] = us
                line("world_frontiers_update", us, face_connected=face, inside_bricks=inside, n_bricks=int(info["n_bricks"]), n_cells=int(info["n_cells"]),
                     n_clusters=int(info["n_clusters"]), largest=sorted(table["n_cells"].tolist(), reverse=True)[:3],
                     n_unknown_faces=int(info["n_unknown_faces"]), n_absent_faces=int(info["n_absent_faces"]))
    # the yardstick: the block's own frontiers (its border is the map's end, like INSIDE_BRICKS)
    for face in (False, True):
        with step("yardstick frontiers_update face=%s" % face, 60):
            def build():
                m.frontiers_update(face_connected=face, max_cells=m.V)
                m.synchronize()
            build()
            us = host_us(build, args.iters)
            table, _ = m.frontiers()
            n_cells = len(m.frontier_cells()[0])
            line("yardstick_frontiers_update", us, face_connected=face, n_cells=n_cells, n_clusters=len(table),
                 world_over_block=round(world_us[(face, True)] / us, 2), world_absent_unknown_over_block=round(world_us[(face, False)] / us, 2))
    m.close()


if __name__ == "__main__":
    main()
