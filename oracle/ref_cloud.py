"""Python side of oracle/ref_cloud_harness.cpp: write a scenario, run the executable of a variant, read the result.

TEST INFRASTRUCTURE ONLY.  The executables are the reference's own generateLabeledPointCloud / manualResize compiled
over oracle/ref_shims/ (`make -C oracle ref`, which needs a checkout of the reference); where oracle/_ref/ is missing,
`exe()` says which file.  Scenario and result are text: integers in decimal, floats as the 8 hex digits of their
binary32 pattern, doubles as the 16 hex digits of their binary64 pattern.

A scenario is a dict:
    noise    (flag, first order, zero order)         the depth-noise flag and the two coefficients
    pose     7 doubles: position, quaternion (w, x, y, z)
    depth    float32 image at sensor size
    entries  list of dicts: track, label (a word; "static" is the static mask), kpts (n x 3 doubles), mask (uint8 image)
"""
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

VARIANTS = ("zed2", "third", "plain", "static")   # oracle/ref_variants/cloud_<variant>.sed


def exe(variant, flavour=None):
    """path of the harness executable of a variant (flavour: None, "O0" or "O3native" of `make ref-spread`)"""
    if flavour:
        return os.path.join(_HERE, "_ref", "spread", "ref_cloud_%s_%s" % (variant, flavour))
    return os.path.join(_HERE, "_ref", "ref_cloud_" + variant)


def _d(values):
    return " ".join("%016x" % int(u) for u in np.ascontiguousarray(values, np.float64).reshape(-1).view(np.uint64))


def _runs(flat, fmt):
    """run-length code of a flat array of integers: 'runs (n v)*'"""
    cut = np.flatnonzero(np.diff(flat)) + 1
    starts = np.concatenate([[0], cut])
    lens = np.diff(np.concatenate([starts, [flat.size]]))
    return "%d %s" % (len(starts), " ".join(("%d " + fmt) % (n, int(flat[s])) for s, n in zip(starts, lens)))


def script(sc):
    """the scenario file of a scenario"""
    flag, first, zero = sc["noise"]
    co = np.array([first, zero], np.float32).view(np.uint32)
    depth = np.ascontiguousarray(sc["depth"], np.float32)
    lines = ["noise %d %08x %08x" % (1 if flag else 0, int(co[0]), int(co[1])), "pose " + _d(sc["pose"]),
             "depth %d %d %s" % (depth.shape[0], depth.shape[1], _runs(depth.reshape(-1).view(np.uint32), "%08x")),
             "entries %d" % len(sc["entries"])]
    for e in sc["entries"]:
        kp = np.asarray(e["kpts"], np.float64).reshape(-1, 3)
        mask = np.ascontiguousarray(e["mask"], np.uint8)
        lines.append("%d %s %d %s %d %d %s" % (e["track"], e["label"], len(kp), _d(kp), mask.shape[0], mask.shape[1],
                                               _runs(mask.reshape(-1), "%d")))
    return "\n".join(lines) + "\n"


def run(variant, text, flavour=None):
    """run one scenario in a process of its own (the reference's label tables are global state) and return the result text"""
    path = exe(variant, flavour)
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "scenario.txt"), os.path.join(d, "result.txt")
        with open(a, "w") as f:
            f.write(text)
        subprocess.run([path, a, b], check=True, stdout=subprocess.DEVNULL, timeout=120)
        with open(b) as f:
            return f.read()


def parse(text):
    """result text -> dict of arrays (what a fixture stores, see FIELDS)"""
    t = text.split()
    at = [0]

    def word():
        at[0] += 1
        return t[at[0] - 1]

    def expect(name):
        w = word()
        if w != name:
            raise ValueError("harness result: %r where %r was expected" % (w, name))

    def ints(n):
        out = np.array([int(x) for x in t[at[0]:at[0] + n]], np.int64)
        at[0] += n
        return out

    def floats(n):
        out = np.array([int(x, 16) for x in t[at[0]:at[0] + n]], np.uint32).view(np.float32)
        at[0] += n
        return out

    r = {}
    expect("variant")
    r["variant"] = ints(5)                      # SETTING, BOOST_MODE, g_consider_instance, width, height
    expect("camera")
    r["camera"] = floats(7)                     # fx fy cx cy depth_min depth_max rescale
    expect("max_movable")
    r["max_movable"] = ints(1)
    expect("sky")
    r["sky"] = ints(1)
    expect("label_to_instance")
    r["label_to_instance"] = ints(int(word()))  # label ids 0 ... 256
    expect("instance_to_label")
    r["instance_to_label"] = ints(2 * int(word())).reshape(-1, 2)
    expect("entry_labels")
    r["entry_labels"] = ints(int(word()))
    expect("depth")
    h, w = int(word()), int(word())
    r["depth"] = floats(h * w).reshape(h, w)
    expect("cloud")
    n = int(word())
    r["pixel"] = np.empty(n, np.int32)
    r["pos"] = np.empty((n, 3), np.float32)
    r["sigma"] = np.zeros(n, np.float32)
    r["clipped"] = np.zeros(n, np.uint8)        # 1: turned into Background by the box filter, sigma left unset
    r["track"] = np.empty(n, np.int32)
    r["label"] = np.empty(n, np.int32)
    for k in range(n):
        r["pixel"][k] = int(word())
        r["pos"][k] = floats(3)
        if t[at[0]] == "--------":
            at[0] += 1
            r["clipped"][k] = 1
        else:
            r["sigma"][k] = floats(1)[0]
        r["track"][k], r["label"][k] = ints(2)
    expect("track_to_label")
    r["track_to_label"] = ints(2 * int(word())).reshape(-1, 2)
    expect("tracked_points")
    r["tracked_points"] = ints(2 * int(word())).reshape(-1, 2)
    expect("end")
    return r


FIELDS = ("variant", "camera", "max_movable", "sky", "label_to_instance", "instance_to_label", "entry_labels", "depth", "pixel",
          "pos", "sigma", "clipped", "track", "label", "track_to_label", "tracked_points")
