"""Times the world objects on the archive of the C3 map (256^3; tools/probes/world_probe.py's: prefilled to ~2 M particles
plus a few frames of the street scene, one sdm_world_update):
  * sdm_world_objects_update, which waits three times, in host microseconds per build (the median of `--iters`), under
    26- and 6-connectivity, without and with BY_TRACK, with the bricks, cells and objects it found;
  * sdm_query_world_objects for 65,536 cells, device mode, between HIP events;
and, in the same process, the yardsticks: sdm_world_frontiers_update on the same archive (host microseconds, the median of
`--iters`), and the NumPy restatement of the tests (tests/world_objects_ref.py's BrickModel) on the bricks of a box of the
archive beside the library's build of the same box (`--model-bricks`: about how many bricks; 0 leaves it out).  One JSON
line each.  Every step runs under a time limit of its own: a step that exceeds it ends the process (SIGALRM's default
action, which no call into the library can hold up), and the line printed before it says which step it was.  Kernel times
come from separate runs, without counters, one connectivity each so that every k_wo_* launch of the trace belongs to it.
On a shared machine every run gets a limit of its own and a failed one ends the chain:

  timeout -k 10 900 python tools/probes/world_objects_probe.py [--iters N] [--frames F] [--model-bricks B] &&
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d OUT26 -- python tools/probes/world_objects_probe.py --only 26 &&
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d OUT6 -- python tools/probes/world_objects_probe.py --only 6
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
from tools.probes.world_frontiers_probe import host_us, step  # noqa: E402
from tools.probes.world_probe import Events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--model-bricks", type=int, default=200)
    ap.add_argument("--only", choices=("26", "6"), help="builds of this connectivity alone, no warm-up of the other, no yardstick")
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
        with step("world_objects_update face=%s alone" % face, 60):
            us = host_us(lambda: m.world_objects_update(face_connected=face), args.iters + 1)
            info = m.world_objects()[1]
            line("world_objects_update", us, face_connected=face, by_track=False, builds=args.iters + 1, n_cells=int(info["n_cells"]))
        m.close()
        return
    with step("warm-up", 60):
        m.world_objects_update()   # code objects, the buffers
        m.world_frontiers_update()
        m.synchronize()
    world_us = {}
    for face in (False, True):
        for by_track in (False, True):
            with step("world_objects_update face=%s by_track=%s" % (face, by_track), 60):
                us = host_us(lambda: m.world_objects_update(face_connected=face, by_track=by_track), args.iters)
                table, info = m.world_objects()
                world_us[(face, by_track)] = us
                line("world_objects_update", us, face_connected=face, by_track=by_track, n_bricks=int(info["n_bricks"]), n_cells=int(info["n_cells"]),
                     n_guessed=int(info["n_guessed"]), n_objects=int(info["n_objects_total"]), largest=sorted(table["n_cells"].tolist(), reverse=True)[:3],
                     ns_per_cell=round(1e3 * us / max(int(info["n_cells"]), 1), 2))
    # the query, device mode, at cells of the last build's list and round them
    with step("query_world_objects 64K", 60):
        ev = Events(m.stream())
        rng = np.random.default_rng(5)
        listed = m.world_object_cells()[0].astype(np.int64)
        n = 65536
        cells = (listed[rng.integers(0, len(listed), n)] + rng.integers(-2, 3, (n, 3))).astype(np.int32)
        d_cells, d_out = m.device_put(cells), m.device_alloc(n * 24)
        query = lambda: m.query_world_objects(cells=d_cells, on_device=True, n=n, out=d_out)  # noqa: E731
        query()
        us = ev.time_us(query, args.iters)
        res = m.device_download(d_out, n * 24, binding.WORLD_OBJECT_RESULT)
        line("query_world_objects_64K", us, cells=n, in_objects=int((res["object"] != binding.WORLD_OBJECT_NONE).sum()), Mcells_per_s=round(n / us, 1))
        m.device_free(d_cells), m.device_free(d_out)
    # the yardsticks: the frontiers of the same archive; the NumPy restatement on the bricks of a box
    for face in (False, True):
        with step("yardstick world_frontiers_update face=%s" % face, 60):
            us = host_us(lambda: m.world_frontiers_update(face_connected=face), args.iters)
            info = m.world_frontiers()[1]
            line("yardstick_world_frontiers_update", us, face_connected=face, n_cells=int(info["n_cells"]), n_clusters=int(info["n_clusters"]),
                 objects_over_frontiers=round(world_us[(face, False)] / us, 2))
    if args.model_bricks > 0:
        with step("yardstick NumPy model on a box", 600):
            from tests import world_objects_ref as wor
            hdr, words = m.world_bricks()
            coord = np.stack([hdr["bx"], hdr["by"], hdr["bz"]], 1).astype(np.int64)
            mid, half = np.median(coord, axis=0).astype(np.int64), 0
            while half < 64 and wor.in_box(coord, (mid - half - 1, mid + half + 1)).sum() <= args.model_bricks:
                half += 1
            box = (tuple(int(v) for v in mid - half), tuple(int(v) for v in mid + half))
            us = host_us(lambda: m.world_objects_update(box=box), args.iters)
            t = time.perf_counter()
            ref = wor.BrickModel(hdr, words, np.float32(cfg["voxel_size"]), cfg["max_movable_track"], box=box, stamp=int(m.world_info()["stamp"]))
            model_us = (time.perf_counter() - t) * 1e6
            got = m.world_object_cells() + m.world_objects()[:1]
            same = wor.difference(got, (ref.cells, ref.object, ref.words, ref.table)) is None
            line("yardstick_numpy_model_box", model_us, n_bricks=int(ref.info["n_bricks"]), n_cells=int(ref.info["n_cells"]),
                 n_objects=int(ref.info["n_objects_total"]), library_us=round(us, 1), model_over_library=round(model_us / us, 1), same_bytes=bool(same))
    m.close()


if __name__ == "__main__":
    main()
