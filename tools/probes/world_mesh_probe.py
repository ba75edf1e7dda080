"""Times the world mesh on the archive of the C3 map (256^3; tools/probes/world_probe.py's: prefilled to ~2 M particles
plus a few frames of the street scene, one sdm_world_update):
  * sdm_world_mesh_update - which waits three times - in host microseconds per build (the median of `--iters`), without a
    box, with a box of a quarter of the archive and with a box of one brick (what the waits and the sort cost when there is
    next to nothing to do), with the bricks, faces, vertex bricks and vertices it found;
  * the fetch of the lists, world_mesh(), in host microseconds;
and, in the same process, the yardsticks: sdm_mesh_update on the block followed by a wait, and what the layer replaces - a
world_bricks() fetch plus tests/world_mesh_ref.py's vectorised model on the same archive, in seconds, its answer compared
with the library's.  One JSON line each.  Every step runs under a time limit of its own: a step that exceeds it ends the
process (SIGALRM's default action), and the line printed before it says which step it was.  Kernel times come from a
separate run, without counters, under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probes/world_mesh_probe.py --only`.

  python tools/probes/world_mesh_probe.py [--iters N] [--frames F] [--only]
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
    ap.add_argument("--only", action="store_true", help="unboxed builds alone: no fetch, no yardstick")
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

    def line(what, us, **kw):
        print(json.dumps(dict({"world": "C3", "what": what, "us": round(us, 1)}, **kw)), flush=True)

    def counts():
        i = m.world_mesh_info()
        return dict(n_bricks=int(i["n_bricks"]), n_faces=int(i["n_faces"]), n_vertex_bricks=int(i["n_vertex_bricks"]), n_vertices=int(i["n_vertices"]),
                    n_solid=int(i["n_solid"]))

    def build_of(**kw):
        def build():
            m.world_mesh_update(**kw)
            m.synchronize()
        return build

    if args.only:
        with step("world_mesh_update alone", 60):
            us = host_us(build_of(), args.iters + 1)
            line("world_mesh_update", us, builds=args.iters + 1, **counts())
        m.close()
        return
    with step("warm-up", 60):
        build_of()()        # code objects, the buffers
        m.mesh_update()
        m.synchronize()
    lo, hi = winfo["bmin"].astype(np.int64), winfo["bmax"].astype(np.int64)
    mid = (lo + hi) // 2
    quarter = (tuple(int(v) for v in lo), (int(mid[0]), int(mid[1]), int(hi[2])))
    hdr = m.world_bricks(with_cells=False)[0]
    one = tuple(int(hdr[len(hdr) // 2][k]) for k in ("bx", "by", "bz"))
    for name, kw in (("whole", {}), ("quarter_box", dict(box=quarter)), ("one_brick_box", dict(box=(one, one))), ("static_skip_unknown", dict(static_only=True, skip_unknown_faces=True))):
        with step("world_mesh_update " + name, 60):
            us = host_us(build_of(**kw), args.iters)
            c = counts()
            line("world_mesh_update", us, field=name, archived=int(winfo["n_bricks"]), ns_per_face=round(1e3 * us / max(c["n_faces"], 1), 2),
                 lists_MB=round((c["n_faces"] * 28 + c["n_vertices"] * 12) / 1e6, 1), **c)
    with step("world_mesh fetch", 60):
        build_of()()
        us = host_us(m.world_mesh, args.iters)
        got = m.world_mesh()
        line("world_mesh_fetch", us, MB=round(sum(np.asarray(got[k]).nbytes for k in ("coords", "faces", "quads", "corners", "xyz")) / 1e6, 1))
    with step("yardstick mesh_update", 60):
        def block():
            m.mesh_update()
            m.synchronize()
        block()
        us = host_us(block, args.iters)
        bi = m.mesh_info()[0]
        line("yardstick_mesh_update", us, cells=int(m.V), n_faces=int(bi["n_faces"]), n_vertices=int(bi["n_vertices"]))
    with step("what it replaces: world_bricks() and the NumPy model", 420):
        from tests import world_mesh_ref as wmr
        t0 = time.perf_counter()
        hdr, cells = m.world_bricks()
        t1 = time.perf_counter()
        ref = wmr.answer(wmr.BrickModel(hdr, cells, cfg["max_movable_track"], stamp=int(winfo["stamp"]), voxel_size=np.float32(cfg["voxel_size"])))
        t2 = time.perf_counter()
        line("numpy_model", (t2 - t0) * 1e6, fetch_s=round(t1 - t0, 3), model_s=round(t2 - t1, 2), same_bytes=wmr.difference(got, ref) is None)
    m.close()


if __name__ == "__main__":
    main()
