"""The HIP library's raw-input path (k_manual_resize, k_labeled_cloud, the staging of frame.hip) against the reference's
own generateLabeledPointCloud, through the fixtures tests/golden/ref_cloud_<variant>.npz (GPU).

Per scenario of tests/ref_cloud_cases.py: one sdm_update_raw_ex on a T0-grid map built from the recorded camera, depth
range and largest movable id, fed with the recorded label table, then sdm_get_labeled_cloud, compared under the rules
stated in tests/ref_cloud_cases.py - the same ones the CPU oracle is held to in tests/test_oracle_cloud_vs_reference.py.
Every scenario runs with host inputs; the scenarios with several object masks run again with the masks back to back
in one buffer (frame.hip's one-transfer path; without BOOST mode only) and with every input resident on the device.
The frame behind the cloud stops after its first stage (the ring shift): what follows does not touch the cloud.
The library has no getter for the reduced depth image; it is held through is_valid at every pixel (every source pixel
that manualResize must not read holds a valid decoy) and through sigma at the valid ones.
Reads only the fixtures and the checkout.
"""
import functools
import os

import numpy as np
import pytest

from oracle import ref_cloud
from tests import ref_cloud_cases as cc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(v, n) for v in ref_cloud.VARIANTS for n in cc.NAMES[v]]
# the other ways in: one per staging path, on the scenarios that have masks to stage
ON_DEVICE = [("zed2", "track_label"), ("third", "max_objects"), ("plain", "plain_boundary"), ("static", "instances_off"), ("zed2", "zero_objects")]
CONTIGUOUS = [("plain", "plain_boundary"), ("plain", "plain_static_movable"), ("static", "instances_off")]


@functools.lru_cache(maxsize=None)
def fixture(variant):
    with np.load(os.path.join(GOLDEN, "ref_cloud_%s.npz" % variant)) as z:
        return {k: z[k] for k in z.files}


def record(variant, name):
    fx = fixture(variant)
    return {k: fx[name + "." + k] for k in ref_cloud.FIELDS}


def run(variant, name, mode):
    from semantic_dsp_map_amd import binding
    sc, rec = cc.scenario(variant, name), record(variant, name)
    a = cc.raw_arguments(sc, rec)
    g = binding.SdmMap(cc.map_config(rec), cc.map_params(sc))
    try:
        objects, static, depth = a["objects"], a["static"], a["depth"]
        held = []
        if mode == "contiguous":
            assert len(objects) > 1 and a["src_size"] is None
            block = np.ascontiguousarray(np.stack([o[2] for o in objects]))
            objects = [(o[0], o[1], block[k]) for k, o in enumerate(objects)]
            assert all(objects[k][2].ctypes.data == objects[k - 1][2].ctypes.data + cc.H * cc.W for k in range(1, len(objects)))
        elif mode == "scattered":      # masks that do not lie back to back: one transfer each
            gap = [np.zeros(o[2].size + 64 * (k + 1), np.uint8) for k, o in enumerate(objects)]
            for buf, o in zip(gap, objects):
                buf[:o[2].size] = o[2].reshape(-1)
            objects = [(o[0], o[1], buf[:o[2].size].reshape(o[2].shape)) for buf, o in zip(gap, objects)]
        elif mode == "device":
            depth = g.device_put(np.ascontiguousarray(depth, np.float32))
            held.append(depth)
            if static is not None:
                static = g.device_put(np.ascontiguousarray(static, np.uint8))
                held.append(static)
            dev = []
            for o in objects:
                p = g.device_put(np.ascontiguousarray(o[2], np.uint8))
                held.append(p)
                dev.append((o[0], o[1], p))
            objects = dev
        g.update_raw(depth, static, a["table"], objects, a["pos"], a["q"], flags=0 if a["consider_instance"] else binding.NO_INSTANCES,
                     stop_after="ego", sync=True, src_size=a["src_size"], rescale=a["rescale"], sky_instance=a["sky_instance"], object_bbox=a["object_bbox"],
                     on_device=mode == "device")
        cloud = g.labeled_cloud()
        for p in held:
            g.device_free(p)
    finally:
        g.close()
    cc.compare(sc, rec, cloud, None, "library, %s inputs" % mode)


@pytest.mark.parametrize("variant,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_library_matches_reference(variant, name):
    run(variant, name, "scattered")


@pytest.mark.parametrize("variant,name", ON_DEVICE, ids=["%s-%s" % c for c in ON_DEVICE])
def test_library_matches_reference_with_inputs_on_the_device(variant, name):
    run(variant, name, "device")


@pytest.mark.parametrize("variant,name", CONTIGUOUS, ids=["%s-%s" % c for c in CONTIGUOUS])
def test_library_matches_reference_with_masks_back_to_back(variant, name):
    run(variant, name, "contiguous")
