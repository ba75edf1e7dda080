"""The life cycle of a map: what sdm_create refuses it refuses before it allocates anything, and what a map allocates -
at creation, or later on demand - goes with it.

The memory figure is the device memory in use as hipMemGetInfo reports it (total - free), read after a device
synchronisation through the HIP runtime the library itself runs on - what torch.cuda.mem_get_info returns where torch sees
the device; in the test process it does not ("No HIP GPUs are available" next to the library's runtime), so the runtime is
asked directly.  That is the whole device's figure: on a card that other processes allocate on during the test it moves
for reasons of theirs.  The tolerance is half of one map's footprint, the footprint being measured here as (in use after
create) - (in use before); a leak smaller than that per cycle is not caught by this test."""
import ctypes as C

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import parity_utils as pu
from tests.test_colour import LABEL_BGR, PERM
from tests.test_labeled_cloud import boost_inputs

pytestmark = pytest.mark.gpu

# 128^3 voxels with 4 slots: the move rows alone are 134 MB, so a map that is left behind is unmistakable
BIG = dict(synth.CONFIGS["T0"], x_n=7, y_n=7, z_n=7, p_n=2)
PARAMS = synth.PARAMS["vkitti2"]


def in_use():
    hip = C.CDLL("libamdhip64.so")  # (already in the process: libsdm_hip.so links it)
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def refused_create(cfg):
    """sdm_create with an image width the row kernel cannot take -> (status, handle)"""
    L = binding.load_library()
    c = binding.Config()
    for k, _ in binding.Config._fields_:
        if k in cfg:
            setattr(c, k, cfg[k])
    c.width, c.shard_count = 4096, 1
    h = C.c_void_p(0xdead)
    return L.sdm_create(C.byref(c), C.byref(h)), h.value


def use_everything(cfg, frames):
    """create; a few frames; every path that allocates on demand; close"""
    g = binding.SdmMap(cfg, PARAMS, synth.noise_table())
    for f in frames[:2]:
        g.update(*f, sync=True)
    for mode in (0, 1, 3, 4, 2):  # every way a plain frame is issued (the first frame after a change is launch by launch)
        g.set_issue_mode(mode)
        for f in frames[2:4]:
            g.update(*f, sync=True)
    p = np.random.default_rng(1).uniform(-3, 3, (1000, 3)).astype(np.float32)
    g.query_points(p, with_index=True)
    g.query_segments(p, p + 1.0)
    g.query_boxes(p, p + 0.5)
    g.esdf_update()
    g.query_distance(p)
    g.occupied()
    g.set_colours(LABEL_BGR, PERM)
    g.occupied_rgb()
    g.tracks_with_particles()
    (sw, sh), depth, static, objects = boost_inputs(cfg)
    g.update_raw(depth, static, synth.LABEL_TO_STATIC_INSTANCE, objects, np.array([0.1, -0.2, 0.3]), np.array([1.0, 0, 0, 0]), sync=True,
                 src_size=(sw, sh), rescale=0.5)
    g.set_params(dict(PARAMS, nb_ptc_num_per_point=3))  # larger birth buffers
    g.update(*frames[4], sync=True)
    g.close()


def test_a_refused_create_leaves_nothing_and_the_next_map_works():
    rc, h = refused_create(BIG)
    assert binding.STATUS_NAMES[rc] == "SDM_ERR_INVALID_ARGUMENT" and h is None
    cfg, params, frames = synth.make_frames("T0", 3, "vkitti2", n_dynamic=2)
    o, g = pu.make_pair(cfg, params, synth.noise_table())
    for t, (depth, cloud, pos, q, moves) in enumerate(frames):
        o.update(depth, cloud, pos, q, moves)
        g.update(depth, cloud, pos, q, moves, sync=True)
        rep = pu.compare_maps(o, g, 1 << cfg["p_n"], tag="frame %d: " % t)
        assert not rep, "\n".join(rep)
    g.close()


def footprint():
    before = in_use()
    g = binding.SdmMap(BIG, PARAMS, synth.noise_table())
    size = in_use() - before
    g.close()
    assert size > 300e6, size  # (the arrays of 128^3 x 4 slots add up to more than that)
    return size


def test_create_use_close_cycles_return_their_memory():
    sc = synth.Scene(BIG, n_dynamic=2, seed=7)
    frames = []
    for t in range(5):
        depth, cloud, pos, q = sc.render(t, PARAMS)
        frames.append((depth, cloud, pos, q, sc.moves(t)))
    use_everything(BIG, frames)  # warm-up: what the runtime keeps for itself is there after this
    size, base = footprint(), in_use()
    for k in range(5):
        use_everything(BIG, frames)
        now = in_use()
        print("cycle %d: %+d bytes against the warm-up cycle (one map: %d)" % (k, now - base, size))
        assert abs(now - base) <= size // 2, (k, now - base, size)


def test_refused_creates_return_their_memory():
    """(A create that checks the width behind its allocations and returns there leaves most of a map behind per attempt.)"""
    size, base = footprint(), in_use()
    for k in range(5):
        rc, h = refused_create(BIG)
        assert binding.STATUS_NAMES[rc] == "SDM_ERR_INVALID_ARGUMENT" and h is None
        now = in_use()
        print("refused create %d: %+d bytes (one map: %d)" % (k, now - base, size))
        assert abs(now - base) <= size // 2, (k, now - base, size)
