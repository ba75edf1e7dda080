"""Times the world changes on the C3 map of the other world probes (256^3; tools/probes/world_probe.py's: prefilled to ~2 M
particles plus a few frames of the street scene).  The map is archived once; the archive is then read back, a known share
of its known cells is altered - occupied cells set free or given another label, free cells set occupied - and imported
again over itself, so that the block, which has not moved, disagrees with its memory in exactly those cells:
  * sdm_world_changes_update, which waits three times, between HIP events round the enqueued calls (so the time holds the
    three waits) and in host microseconds (the median of `--iters`), under 26- and 6-connectivity, without and with
    BY_LABEL, with the candidates, bricks, cells and regions it found, the bytes it has to move - the result lines of the
    block and the archived bricks the block overlaps, once each - and the rate that implies;
  * the same with all-zero masks: the comparison and its counters alone, one wait;
  * sdm_query_world_changes for 65,536 cells, device mode;
and, in the same process, the yardsticks: sdm_world_update (between HIP events) and sdm_world_objects_update (host
microseconds and between HIP events) on the same archive.  One JSON line each.  Every step runs under a time limit of its
own: a step that exceeds it ends the process (SIGALRM's default action), and the line printed before it says which.

  timeout -k 10 900 python tools/probes/world_changes_probe.py [--iters N] [--frames F] [--share S]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_dsp_map_amd import binding, synth  # noqa: E402
from tools.probes.world_frontiers_probe import host_us, step  # noqa: E402
from tools.probes.world_probe import Events  # noqa: E402


def altered(cells, share, seed=11):
    """a copy of the archived words with `share` of the known ones changed -> (words, how many were changed)"""
    rng = np.random.default_rng(seed)
    out = cells.copy()
    occ = (cells >> 24).astype(np.uint8).view(np.int8)
    known = np.flatnonzero(occ.reshape(-1) >= 0)
    pick = rng.choice(known, int(len(known) * share), replace=False)
    flat = out.reshape(-1)
    was = occ.reshape(-1)[pick]
    kind = rng.integers(0, 2, len(pick))
    wall = np.uint32(1 << 24 | synth.LABEL_BUILDING << 16 | synth.TRACK_BUILDING)
    relabel = (flat[pick] & np.uint32(0xFF00FFFF)) | (((flat[pick] >> 16) + 1) & np.uint32(0xFF)) << np.uint32(16)
    flat[pick] = np.where(was == 0, wall, np.where(kind == 0, np.uint32(0), relabel)).astype(np.uint32)
    return out, len(pick)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--share", type=float, default=0.01)
    args = ap.parse_args()
    cfg, params = synth.CONFIGS["C3"], synth.PARAMS["vkitti2"]
    with step("the C3 map, its archive and the altered memory", 300):
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
        hdr, cells = m.world_bricks()
        other, n_altered = altered(cells, args.share)
        m.world_import(hdr, other)
        m.synchronize()
    w = binding.WorldChanges(m)
    ev = Events(m.stream())
    V = m.V

    def line(what, us, **kw):
        print(json.dumps(dict({"world": "C3", "what": what, "us": round(us, 1)}, **kw)), flush=True)

    with step("warm-up", 120):
        w.update()   # code objects, the buffers
        m.world_objects_update()
        m.synchronize()
        info = w.regions()[1]
        line("altered", 0.0, share=args.share, cells_altered=n_altered, n_cells=int(info["n_cells"]), archived_bricks=len(hdr))
    moved = 2 * V * 4 + len(hdr) * 2048     # the 8-byte result lines of the block, the archived bricks it overlaps
    for face in (False, True):
        for by_label in (False, True):
            with step("world_changes_update face=%s by_label=%s" % (face, by_label), 120):
                build = lambda: w.update(face_connected=face, by_label=by_label)  # noqa: E731
                host = host_us(build, args.iters)
                us = ev.time_us(build, args.iters)
                table, info = w.regions()
                line("world_changes_update", us, host_us=round(host, 1), face_connected=face, by_label=by_label,
                     n_candidates=int(info["n_candidates"]), n_bricks=int(info["n_bricks"]), n_cells=int(info["n_cells"]),
                     n_regions=int(info["n_regions_total"]), largest=sorted(table["n_cells"].tolist(), reverse=True)[:3],
                     appeared=int(info["n_appeared"]), vanished=int(info["n_vanished"]), relabelled=int(info["n_relabelled"]),
                     bytes_moved=moved, TBps=round(moved / us / 1e6, 3))
    with step("world_changes_update, nothing listed", 120):
        build = lambda: w.update(classes=())  # noqa: E731
        host = host_us(build, args.iters)
        us = ev.time_us(build, args.iters)
        line("world_changes_update_counters_only", us, host_us=round(host, 1), bytes_moved=moved, TBps=round(moved / us / 1e6, 3))
    with step("query_world_changes 64K", 60):
        w.update()
        got = w.cells()[0]
        rng = np.random.default_rng(3)
        n = 1 << 16
        pick = got[rng.integers(0, len(got), n)].astype(np.int32) + rng.integers(-1, 2, (n, 3)).astype(np.int32)
        d_in, d_out = m.device_put(pick), m.device_alloc(n * 24)
        query = lambda: w.query(cells=d_in, on_device=True, n=n, out=d_out)  # noqa: E731
        query()
        us = ev.time_us(query, args.iters)
        res = m.device_download(d_out, n * 24, binding.WORLD_CHANGE_RESULT)
        line("query_world_changes_64K", us, cells=n, listed=int((res["region"] != binding.WORLD_CHANGE_NONE).sum()), Mcells_per_s=round(n / us, 1))
        m.device_free(d_in), m.device_free(d_out)
    with step("yardstick: world_objects_update", 120):
        host = host_us(m.world_objects_update, args.iters)
        us = ev.time_us(m.world_objects_update, args.iters)
        oinfo = m.world_objects()[1]
        line("yardstick_world_objects_update", us, host_us=round(host, 1), n_cells=int(oinfo["n_cells"]), n_objects=int(oinfo["n_objects_total"]))
    with step("yardstick: world_update", 120):
        us = ev.time_us(m.world_update, args.iters)     # (last: it writes the block over the altered memory)
        line("yardstick_world_update", us, bytes_moved=moved, TBps=round(moved / us / 1e6, 3))
    m.close()


if __name__ == "__main__":
    main()
