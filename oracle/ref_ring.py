"""Python side of oracle/ref_harness.cpp: write a scenario, run the executable of a variant, read the result.

TEST INFRASTRUCTURE ONLY.  The executables are the reference's own ring buffer compiled over oracle/ref_shims/
(`make -C oracle ref`, which needs a checkout of the reference); where oracle/_ref/ is missing, `exe()` says which file.
Scenario and result are text: integers in decimal, floats as the 8 hex digits of their binary32 pattern.
"""
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

# variant of settings/settings.h (oracle/ref_variants/<variant>.sed) -> the project's configuration of the same numbers
VARIANTS = {"zed2_boost": "REF_ZED2_BOOST", "t1": "T1", "t0": "T0"}
STATE_KEYS = ("idx", "px", "py", "pz", "w", "ts", "track", "label", "status", "forget")


def exe(variant, flavour=None):
    """path of the harness executable of a variant (flavour: None, "O0" or "O3native" of `make ref-spread`)"""
    if flavour:
        return os.path.join(_HERE, "_ref", "spread", "ref_ring_%s_%s" % (variant, flavour))
    return os.path.join(_HERE, "_ref", "ref_ring_" + variant)


def fhex(v):
    return "%08x" % int(np.asarray(v, np.float32).reshape(()).view(np.uint32))


def _fl(a):
    return " ".join("%08x" % int(u) for u in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


class Script:
    """the commands of one scenario, in the order the harness runs them"""

    def __init__(self):
        self.lines = []

    def text(self):
        return "\n".join(self.lines) + "\n"

    def noise(self, values):
        v = np.atleast_1d(np.asarray(values, np.float32))
        self.lines.append("noise %d %s" % (v.size, _fl(v)))

    def ts(self, t):
        self.lines.append("ts %d" % t)

    def ego(self, pos):
        self.lines.append("ego " + _fl(pos))

    def load(self, sp):
        """sp: sparse state, a dict of equally long arrays under STATE_KEYS"""
        self.lines.append("load %d" % len(sp["idx"]))
        for k in range(len(sp["idx"])):
            self.lines.append(" %d %s %d %d %d %d %d" % (sp["idx"][k], _fl([sp["px"][k], sp["py"][k], sp["pz"][k], sp["w"][k]]),
                                                         sp["ts"][k], sp["track"][k], sp["label"][k], sp["status"][k], sp["forget"][k]))

    def pos_to_voxel(self, pts):
        p = np.asarray(pts, np.float32).reshape(-1, 3)
        self.lines.append("pos_to_voxel %d %s" % (len(p), _fl(p)))

    def voxel_to_pos(self, voxels):
        self.lines.append("voxel_to_pos %d %s" % (len(voxels), " ".join(str(int(v)) for v in voxels)))

    def add(self, pts, label, track, guessed=False):
        p = np.asarray(pts, np.float32).reshape(-1, 3)
        self.lines.append("add %d %d %d %d %s" % (1 if guessed else 0, label, track, len(p), _fl(p)))

    def move(self, sets, matrices):
        self.lines.append("move %d" % len(sets))
        for s, m in zip(sets, matrices):
            self.lines.append(" %s %d %s" % (_fl(m), len(s), " ".join(str(int(i)) for i in s)))

    def delete(self, indices):
        self.lines.append("delete %d %s" % (len(indices), " ".join(str(int(i)) for i in indices)))

    def visible(self, extrinsic, depth, multi_threaded=False):
        d = np.ascontiguousarray(depth, np.float32).reshape(-1).view(np.uint32)
        cut = np.flatnonzero(np.diff(d)) + 1
        starts = np.concatenate([[0], cut])
        lens = np.diff(np.concatenate([starts, [d.size]]))
        runs = " ".join("%d %08x" % (n, int(d[s])) for s, n in zip(starts, lens))
        self.lines.append("visible %d %s %d %s" % (1 if multi_threaded else 0, _fl(extrinsic), len(starts), runs))

    def frustum(self, extrinsic, pts):
        p = np.asarray(pts, np.float32).reshape(-1, 3)
        self.lines.append("frustum %s %d %s" % (_fl(extrinsic), len(p), _fl(p)))

    def occupancy(self, threshold):
        self.lines.append("occupancy " + fhex(threshold))

    def fusion(self, voxels, threshold, neighbours=False):
        self.lines.append("fusion %d %s %d %s" % (1 if neighbours else 0, fhex(threshold), len(voxels), " ".join(str(int(v)) for v in voxels)))

    def pdf_table(self):
        self.lines.append("pdf_table")

    def query_pdf(self, x_mu_sigma):
        a = np.asarray(x_mu_sigma, np.float32).reshape(-1, 3)
        self.lines.append("query_pdf %d %s" % (len(a), _fl(a)))

    def forgetting_factor(self, stability, max_count, counts):
        self.lines.append("forgetting_factor %s %d %d %s" % (fhex(stability), max_count, len(counts), " ".join(str(int(c)) for c in counts)))

    def dump(self, *what):
        for w in what:
            self.lines.append("dump_" + w)


def run(variant, text, flavour=None, path=None):
    """run one scenario in a process of its own (the reference's map is global state) and return the result text"""
    path = path or exe(variant, flavour)
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "scenario.txt"), os.path.join(d, "result.txt")
        with open(a, "w") as f:
            f.write(text)
        subprocess.run([path, a, b], check=True, stdout=subprocess.DEVNULL, timeout=120)
        with open(b) as f:
            return f.read()


class _Tokens:
    def __init__(self, text):
        self.t = text.split()
        self.i = 0

    def word(self):
        self.i += 1
        return self.t[self.i - 1]

    def ints(self, n, dtype=np.int64):
        out = np.array([int(x) for x in self.t[self.i:self.i + n]], dtype)
        self.i += n
        return out

    def floats(self, n):
        out = np.array([int(x, 16) for x in self.t[self.i:self.i + n]], np.uint32).view(np.float32)
        self.i += n
        return out

    def int(self):
        return int(self.word())


def parse(text):
    """result text -> list of (name, value) in the order the harness wrote them"""
    tk = _Tokens(text)
    out = []
    while True:
        name = tk.word()
        if name == "end":
            return out
        if name == "variant":
            v = tk.ints(6)
            out.append((name, {"n": v[:3].tolist(), "slots": int(v[3]), "width": int(v[4]), "height": int(v[5])}))
        elif name == "camera":
            out.append((name, tk.floats(7)))
        elif name == "pos_to_voxel":
            out.append((name, tk.ints(tk.int(), np.uint32)))
        elif name == "voxel_to_pos":
            out.append((name, tk.floats(3 * tk.int()).reshape(-1, 3)))
        elif name == "add":
            out.append((name, tk.ints(2 * tk.int(), np.uint32).reshape(-1, 2)))
        elif name == "move":
            out.append((name, [tk.ints(tk.int(), np.uint32) for _ in range(tk.int())]))
        elif name == "visible":
            out.append((name, tk.int()))
        elif name == "frustum":
            out.append((name, tk.ints(tk.int(), np.uint8)))
        elif name == "occupancy":
            unknown, n = tk.int(), tk.int()
            out.append((name, {"unknown": unknown, "rows": tk.ints(4 * n).reshape(-1, 4)}))
        elif name == "fusion":
            n = tk.int()
            rows = {"wsum": np.empty(n, np.float32), "guessed": np.empty(n, np.float32), "label": np.empty(n, np.int64), "track": np.empty(n, np.int64)}
            for k in range(n):
                rows["wsum"][k], rows["guessed"][k] = tk.floats(2)
                rows["label"][k], rows["track"][k] = tk.ints(2)
            out.append((name, rows))
        elif name in ("pdf_table", "query_pdf", "forgetting_factor"):
            out.append((name, tk.floats(tk.int())))
        elif name == "ring":
            v = tk.ints(7)
            f = tk.floats(6)
            out.append((name, {"global_time_stamp": int(v[0]), "moved_steps": v[1:4].tolist(), "eq_steps": v[4:7].tolist(),
                               "map_center": f[:3].copy(), "last_pos": f[3:].copy()}))
        elif name == "stamps":
            n = tk.ints(3)
            out.append((name, tuple(tk.ints(int(k), np.uint32) for k in n)))
        elif name in ("state", "particles"):      # particles: the same rows without the time slots (ref_filter_harness.cpp)
            n = tk.int()
            sp = {"idx": np.empty(n, np.int64), "px": np.empty(n, np.float32), "py": np.empty(n, np.float32), "pz": np.empty(n, np.float32),
                  "w": np.empty(n, np.float32), "ts": np.empty(n, np.int64), "track": np.empty(n, np.int64), "label": np.empty(n, np.int64),
                  "status": np.empty(n, np.int64), "forget": np.empty(n, np.int64)}
            for k in range(n):
                sp["idx"][k] = tk.int()
                sp["px"][k], sp["py"][k], sp["pz"][k], sp["w"][k] = tk.floats(4)
                sp["ts"][k], sp["track"][k], sp["label"][k], sp["status"][k], sp["forget"][k] = tk.ints(5)
            out.append((name, sp))
        elif name == "births":        # oracle/ref_filter_harness.cpp: added_particle_num, the resampled voxels in ascending order
            added, n = tk.int(), tk.int()
            out.append((name, {"added": added, "resampled": tk.ints(n, np.uint32)}))
        elif name == "resample":
            out.append((name, tk.ints(tk.int(), np.uint8)))
        elif name == "cursor":
            out.append((name, tk.int()))
        elif name == "owners":
            owners = {}
            for _ in range(tk.int()):
                track, n = tk.int(), tk.int()
                owners[track] = tk.ints(n, np.uint32)
            out.append((name, owners))
        elif name == "bins":
            bins = {}
            for _ in range(tk.int()):
                pid, n = tk.int(), tk.int()
                bins[pid] = tk.ints(n, np.uint32)
            out.append((name, bins))
        else:
            raise ValueError("unknown record %r in a harness result" % name)


def first(records, name, k=0):
    """the k-th record of a name"""
    return [v for n, v in records if n == name][k]
