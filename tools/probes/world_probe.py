"""Times the world archive on the C3 map (256^3): prefilled to ~2 M particles (synth.prefill_state) plus a few frames of the
street scene.  Every time is taken with HIP events recorded on the map's stream around the calls, which only enqueue:
  * the first sdm_world_update after sdm_world_clear, in which every brick is created (`--iters` times: clear, update);
  * the one update after the camera has moved by one cell (a slab of new bricks at most), and `--iters` updates of that
    frame issued back to back - the steady state: every brick exists, every observed cell is stored again;
  * sdm_query_world_points for 1 M points inside the archive's bounds, device mode;
  * sdm_get_world_region of a 256^3 box around the block, device mode;
and, in the same process, sdm_mesh_update and sdm_esdf_update as yardsticks that stream the same result array.
One JSON line each, with the bytes the update moves: it reads the second result word of every cell of the block twice
(k_world_mark, k_world_merge: 4 B x V each; the 8-byte results are fetched in 64-byte lines either way, so the line
traffic is twice that), and per brick with a writing cell it writes 2 KB when the brick is new and reads 2 KB and stores
the writing cells again when it is archived.

  python tools/probes/world_probe.py [--iters N] [--frames F]
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

HIP = C.CDLL("libamdhip64.so")


def hip(rc):
    if rc != 0:
        raise RuntimeError("HIP error %d" % rc)


class Events:
    """a pair of events on one stream: the time between them, on the device"""

    def __init__(self, stream):
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        hip(HIP.hipEventCreate(C.byref(self.a)))
        hip(HIP.hipEventCreate(C.byref(self.b)))

    def time_us(self, fn, iters=1, before=None):
        """fn() `iters` times between the two events (before(): enqueued ahead of each, outside the window when iters is 1)"""
        total = 0.0
        rounds = 1 if before is None else iters
        for _ in range(rounds):
            if before is not None:
                before()
            hip(HIP.hipEventRecord(self.a, self.stream))
            for _ in range(iters if before is None else 1):
                fn()
            hip(HIP.hipEventRecord(self.b, self.stream))
            hip(HIP.hipEventSynchronize(self.b))
            ms = C.c_float()
            hip(HIP.hipEventElapsedTime(C.byref(ms), self.a, self.b))
            total += ms.value * 1e3
        return total / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4)
    args = ap.parse_args()
    cfg, params = synth.CONFIGS["C3"], synth.PARAMS["vkitti2"]
    scene = synth.Scene(cfg, n_static=48, n_dynamic=6, seed=7)
    st, ring, n_pre = synth.prefill_state(cfg, scene, 2000000)
    m = binding.SdmMap(cfg, params, synth.noise_table())
    m.load_state(st)
    m.set_ring_state(ring)
    pos = q = None
    for t in range(args.frames):
        depth, cloud, pos, q = scene.render(t, params)
        m.update(depth, cloud, pos, q, scene.moves(t))
    m.synchronize()
    V, size = m.V, np.float32(cfg["voxel_size"])
    ev = Events(m.stream())
    vox = m.voxels()
    observed = int((vox["occ"] >= 0).sum())

    def line(what, us, **kw):
        print(json.dumps(dict({"world": "C3", "what": what, "voxels": V, "us": round(us, 1)}, **kw)), flush=True)

    def update_line(what, us, info, written_bytes, read_bytes):
        words = 2 * V * 4
        line(what, us, n_bricks=int(info["n_bricks"]), created=int(info["created_last"]), dropped=int(info["dropped_last"]),
             observed_cells=observed, word_bytes=words, brick_bytes_written=written_bytes, brick_bytes_read=read_bytes,
             word_TBps=round(words / us / 1e6, 3), line_TBps=round(2 * words / us / 1e6, 3),
             total_TBps=round((2 * words + written_bytes + read_bytes) / us / 1e6, 3))

    # warm-up: code objects, the buffers
    m.world_update()
    m.world_info()
    # the first update: every brick is created
    us = ev.time_us(m.world_update, args.iters, before=m.world_clear)
    info = m.world_info()
    update_line("first_update", us, info, int(info["n_bricks"]) * 2048, 0)
    # one cell further: the update that creates the new slab's bricks, then the steady state
    step = np.array([size, 0, 0], np.float32)
    depth, cloud, _, _ = scene.render(args.frames, params)
    m.update(depth, cloud, pos + step, q, scene.moves(args.frames), sync=True)
    observed = int((m.voxels()["occ"] >= 0).sum())
    us = ev.time_us(m.world_update)
    info = m.world_info()
    bricks = int(info["n_bricks"])
    update_line("update_after_one_cell_shift", us, info, int(info["created_last"]) * 2048 + observed * 4, (bricks - int(info["created_last"])) * 2048)
    us = ev.time_us(m.world_update, args.iters)
    info = m.world_info()
    update_line("steady_update", us, info, observed * 4, bricks * 2048)
    # the queries, device mode
    n = 1 << 20
    rng = np.random.default_rng(5)
    lo, hi = info["bmin"].astype(np.float64) * 8, (info["bmax"].astype(np.float64) + 1) * 8
    xyz = ((rng.uniform(lo, hi, (n, 3)).astype(np.int64).astype(np.float32) + np.float32(0.5)) * size).astype(np.float32)
    d_xyz, d_out = m.device_put(xyz), m.device_alloc(n * 8)
    query = lambda: m.query_world(d_xyz, on_device=True, n=n, out=d_out)  # noqa: E731
    query()
    us = ev.time_us(query, args.iters)
    hit = int((m.device_download(d_out, n * 8, binding.WORLD_CELL)["occ"] >= 0).sum())
    line("query_world_1M", us, points=n, answered=hit, Mpoints_per_s=round(n / us, 1))
    box = np.array([256, 256, 256], np.int64)
    cell_min = np.array(m.ring_state()["moved_steps"], np.int64) - 128
    d_words = m.device_alloc(int(box.prod()) * 4)
    region = lambda: m.world_region(cell_min, box, on_device=True, out=d_words)  # noqa: E731
    region()
    us = ev.time_us(region, args.iters)
    line("world_region_256^3", us, words=int(box.prod()), out_TBps=round(int(box.prod()) * 4 / us / 1e6, 3))
    # the yardsticks: two builds that stream the same result array
    for name, fn in (("mesh_update", m.mesh_update), ("esdf_update", m.esdf_update)):
        fn()
        m.synchronize()
        us = ev.time_us(fn, args.iters)
        line("yardstick_" + name, us, word_bytes=V * 4, word_TBps=round(V * 4 / us / 1e6, 3), line_TBps=round(V * 8 / us / 1e6, 3))
    for p in (d_xyz, d_out, d_words):
        m.device_free(p)
    m.close()


if __name__ == "__main__":
    main()
