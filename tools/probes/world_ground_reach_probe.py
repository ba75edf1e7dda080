"""Times world ground reach on the archive of the C3 map (256^3; tools/probes/world_probe.py's: prefilled to ~2 M particles
plus a few frames of the street scene, one sdm_world_update) over the ground layer of tools/probes/world_ground_probe.py's
settings (up axis (1, -1), a band of 64 cells from the archive's lowest cell, clearance 4, R = 8):
  * sdm_world_ground_reach_update (it waits) from one start, the ground column nearest to the middle of the layer, 8- and
    4-connected, with and without a budget and a min_d2, in host microseconds per build (the median of `--iters`), with the
    rounds, the tiles relaxed over all rounds, the columns reached and the microseconds per tile visit; then the same
    builds over a second ground layer of the same archive ("open": every label carries, unknown cells passable, clearance
    1, no step lethal) under max_climb 65535, from a column of its largest 4-connected patch of ground: 5q's settings
    leave this scene - prefilled particles, not a street - a scatter of ground columns, and the field of that layer stays
    where it starts;
  * sdm_query_world_ground_reach for 65,536 goals and sdm_world_ground_reach_paths for 1,024 goals, device mode, between
    HIP events;
and, in the same process on the same archive, the two yardsticks: sdm_world_ground_update followed by a wait, and
sdm_world_reach_update (face-connected, through unknown cells, from the same place) with its rounds and bricks relaxed, and
the ratios.  One JSON line each, printed and written to `--out` (by default profiles/world_ground_reach_probe.txt, which
the run replaces).  Every step runs under a time limit of its own (tools/probes/world_esdf_probe.py's `step`).

  python tools/probes/world_ground_reach_probe.py [--iters N] [--frames F] [--out FILE]
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

UP = (1, -1)
BAND = 64
RADIUS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_ground_reach_probe.txt"))
    args = ap.parse_args()
    out = open(args.out, "w")
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
    n_arch = int(winfo["n_bricks"])
    g_max, g_min = (int(winfo["bmax"][UP[0]]) + 1) * 8 - 1, int(winfo["bmin"][UP[0]]) * 8
    h_lo = g_min if UP[1] > 0 else -1 - g_max
    gopts = dict(up=UP, h_lo=h_lo, h_hi=h_lo + BAND - 1, clearance=4, max_step=1, radius=RADIUS, support_labels=[synth.LABEL_ROAD])
    a, au, av = UP[0], (1 if UP[0] == 0 else 0), (1 if UP[0] == 2 else 2)

    def line(what, us, **kw):
        text = json.dumps(dict({"world": "C3", "what": what, "us": round(us, 1)}, **kw))
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    def ground():
        m.world_ground_update(**gopts)
        m.synchronize()

    with step("the ground layer and the start", 60):
        ground()
        coords, cells, d2, ginfo = m.world_ground()
        tiles = int(ginfo["n_tiles"])
        ok = (cells["cls"] & 11) == 1                                   # ground, not lethal
        r, w = np.nonzero(ok)
        iu, iv = coords[r, 0].astype(np.int64) * 8 + (w & 7), coords[r, 1].astype(np.int64) * 8 + (w >> 3)
        k = int(np.argmin((iu - np.median(iu)) ** 2 + (iv - np.median(iv)) ** 2))
        start = np.zeros((1, 3), np.int32)
        start[0, au], start[0, av] = iu[k], iv[k]
        level = int(cells["level"][r[k], w[k]])
        h = h_lo + level + 1
        start[0, a] = h if UP[1] > 0 else -1 - h

    variants = [("8-connected", dict(max_climb=1)), ("4-connected", dict(max_climb=1, face_connected=True)),
                ("8-connected, max_cost 2000", dict(max_climb=1, max_cost=2000)), ("8-connected, min_d2 4", dict(max_climb=1, min_d2=4)),
                ("8-connected, min_d2 4, soft_d2 16, penalty 5", dict(max_climb=1, min_d2=4, soft_d2=16, penalty=5)),
                ("4-connected, min_d2 4, max_cost 2000", dict(max_climb=1, face_connected=True, min_d2=4, max_cost=2000))]
    with step("warm-up", 120):
        for _, kw in variants[:2]:
            m.world_ground_reach_update(start_cells=start, **kw)
        m.world_reach_update(start_cells=start, face_connected=True, through_unknown=True)
    reach_us = {}
    for name, kw in variants:
        with step("world_ground_reach_update " + name, 120):
            us = host_us(lambda: m.world_ground_reach_update(start_cells=start, **kw), args.iters)
            info = m.world_ground_reach(with_cost=False, cap=0)[2]
            visits = m.world_ground_reach_tiles_relaxed()
            reach_us[name] = us
            line("world_ground_reach_update", us, variant=name, n_tiles=int(info["n_tiles"]), n_traversable=int(info["n_traversable"]),
                 n_reached=int(info["n_reached"]), max_cost_reached=int(info["max_cost_reached"]), rounds=int(info["rounds"]), tiles_relaxed=visits,
                 us_per_round=round(us / max(int(info["rounds"]), 1), 2), us_per_tile_visit=round(us / max(visits, 1), 3))
    # the open ground: the same archive, every label carries, no step lethal, every climb allowed - a field that spreads;
    # the start: a column of the largest 4-connected patch of ground columns, found on the host
    open_opts = dict(gopts, max_step=65535, clearance=1, support_labels=list(range(256)), unknown_passable=True)
    with step("the open ground layer and its start", 120):
        m.world_ground_update(**open_opts)
        coords, cells, d2, oinfo = m.world_ground()
        u0, v0 = int(coords[:, 0].min()) * 8, int(coords[:, 1].min()) * 8
        grid = np.zeros(((int(coords[:, 1].max()) + 1) * 8 - v0, (int(coords[:, 0].max()) + 1) * 8 - u0), bool)
        level = np.zeros(grid.shape, np.int64)
        for r, (bu, bv) in enumerate(coords.astype(np.int64).tolist()):
            sl = (slice(8 * bv - v0, 8 * bv - v0 + 8), slice(8 * bu - u0, 8 * bu - u0 + 8))
            grid[sl], level[sl] = ((cells["cls"][r] & 11) == 1).reshape(8, 8), cells["level"][r].reshape(8, 8)
        seen, best = np.zeros(grid.shape, bool), []
        for y, x in np.argwhere(grid).tolist():
            if seen[y, x]:
                continue
            patch, todo = [], [(y, x)]
            seen[y, x] = True
            while todo:
                cy, cx = todo.pop()
                patch.append((cy, cx))
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < grid.shape[0] and 0 <= nx < grid.shape[1] and grid[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        todo.append((ny, nx))
            if len(patch) > len(best):
                best = patch
        sy, sx = best[len(best) // 2]
        h = h_lo + int(level[sy, sx]) + 1
        start = np.zeros((1, 3), np.int32)
        start[0, au], start[0, av], start[0, a] = sx + u0, sy + v0, (h if UP[1] > 0 else -1 - h)
        line("open_ground_layer", 0.0, n_tiles=int(oinfo["n_tiles"]), n_ground=int(oinfo["n_ground"]), n_lethal=int(oinfo["n_lethal"]),
             largest_patch=len(best))
    C = 65535
    open_variants = [("open, 8-connected", dict(max_climb=C)), ("open, 4-connected", dict(max_climb=C, face_connected=True)),
                     ("open, 8-connected, max_cost 500", dict(max_climb=C, max_cost=500)),
                     ("open, 8-connected, min_d2 2, soft_d2 16, penalty 5", dict(max_climb=C, min_d2=2, soft_d2=16, penalty=5))]
    for name, kw in open_variants:
        with step("world_ground_reach_update " + name, 120):
            us = host_us(lambda: m.world_ground_reach_update(start_cells=start, **kw), args.iters)
            info = m.world_ground_reach(with_cost=False, cap=0)[2]
            visits = m.world_ground_reach_tiles_relaxed()
            reach_us[name] = us
            line("world_ground_reach_update", us, variant=name, n_tiles=int(info["n_tiles"]), n_traversable=int(info["n_traversable"]),
                 n_reached=int(info["n_reached"]), max_cost_reached=int(info["max_cost_reached"]), rounds=int(info["rounds"]), tiles_relaxed=visits,
                 us_per_round=round(us / max(int(info["rounds"]), 1), 2), us_per_tile_visit=round(us / max(visits, 1), 3))
    with step("yardstick world_ground_update", 60):
        us_ground = host_us(ground, args.iters)
        line("yardstick_world_ground_update", us_ground, n_tiles=tiles, n_archived_bricks=n_arch,
             reach_over_ground=round(reach_us["8-connected"] / us_ground, 2), open_reach_over_ground=round(reach_us["open, 8-connected"] / us_ground, 2))
    with step("yardstick world_reach_update", 240):
        us_wr = host_us(lambda: m.world_reach_update(start_cells=start, face_connected=True, through_unknown=True), max(args.iters // 3, 1))
        winfo_r = m.world_reach(with_cost=False, cap=0)[2]
        bricks = m.world_reach_bricks_relaxed()
        line("yardstick_world_reach_update", us_wr, n_bricks=int(winfo_r["n_bricks"]), n_reached=int(winfo_r["n_reached"]), rounds=int(winfo_r["rounds"]),
             bricks_relaxed=bricks, us_per_round=round(us_wr / max(int(winfo_r["rounds"]), 1), 2), us_per_brick_visit=round(us_wr / max(bricks, 1), 3),
             world_reach_over_ground_reach_4=round(us_wr / reach_us["4-connected"], 2),
             world_reach_over_open_ground_reach_4=round(us_wr / reach_us["open, 4-connected"], 2))
    # the queries, device mode, on the open 8-connected field
    with step("queries", 120):
        m.world_ground_update(**open_opts)
        m.world_ground_reach_update(start_cells=start, **open_variants[0][1])
        ev = Events(m.stream())
        rng = np.random.default_rng(5)
        lo, hi = winfo["bmin"].astype(np.float64) * 8, (winfo["bmax"].astype(np.float64) + 1) * 8
        n = 65536
        goals = rng.uniform(lo, hi, (n, 3)).astype(np.int32)
        d_in, d_out = m.device_put(goals), m.device_alloc(n * 24)
        query = lambda: m.query_world_ground_reach(cells=d_in, on_device=True, n=n, out=d_out)  # noqa: E731
        query()
        us = ev.time_us(query, args.iters)
        res = m.device_download(d_out, n * 24, binding.WORLD_GROUND_REACH_RESULT)
        line("query_world_ground_reach_64K", us, goals=n, reached=int((res["status"] == 0).sum()), in_tiles=int((res["status"] != 3).sum()),
             Mgoals_per_s=round(n / us, 1))
        k, max_len = 1024, 1024
        pick = goals[np.flatnonzero(res["status"] == 0)[:k]]
        assert len(pick) > 0
        pick = np.ascontiguousarray(np.resize(pick, (k, 3)))
        d_goals, d_rows, d_lens = m.device_put(pick), m.device_alloc(k * max_len * 12), m.device_alloc(k * 4)
        paths = lambda: m.world_ground_reach_paths(cells=d_goals, max_len=max_len, on_device=True, n=k, cells_out=d_rows, len_out=d_lens)  # noqa: E731
        paths()
        us = ev.time_us(paths, args.iters)
        lens = m.device_download(d_lens, k * 4, np.int32)
        line("world_ground_reach_paths_1K", us, goals=k, cells=int(lens.sum()), longest=int(lens.max()), ns_per_cell=round(1e3 * us / max(int(lens.sum()), 1), 1))
        for p in (d_in, d_out, d_goals, d_rows, d_lens):
            m.device_free(p)
    m.close()
    out.close()


if __name__ == "__main__":
    main()
