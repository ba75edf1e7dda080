"""Writes tests/golden/ref_ring_<variant>.npz: for every scenario of tests/ref_ring_cases.py the commands given to the
reference harness (oracle/ref_harness.cpp over the reference's own ring buffer) and the text it answered.

Needs the executables of `make -C oracle ref`, hence a checkout of the reference; the tests need only the fixtures.

    python -m tests.golden.make_golden_ref_ring            # write the fixtures
    python -m tests.golden.make_golden_ref_ring --spread   # after `make -C oracle ref-spread`: the float spread between
                                                           # an -O0 and an -O3 -march=native build of the harness
"""
import os
import sys

import numpy as np

from oracle import ref_ring
from tests import ref_ring_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))


def path(variant):
    return os.path.join(HERE, "ref_ring_%s.npz" % variant)


def runs(variant, sc, flavour=None):
    """[(key, commands, answer)] of a scenario"""
    text = rc.script(sc)
    out = [("", text, ref_ring.run(variant, text, flavour))]
    if sc["kind"] == "index":       # voxel -> position needs the voxels the first run found
        voxels = ref_ring.first(ref_ring.parse(out[0][2]), "pos_to_voxel")
        text2 = rc.index_script_tail(sc, np.unique(voxels[voxels != 0xffffffff]))
        out.append(("2", text2, ref_ring.run(variant, text2, flavour)))
    return out


def as_bytes(text):
    return np.frombuffer(text.encode("ascii"), np.uint8)


def write():
    for variant in ref_ring.VARIANTS:
        data = {}
        for sc in rc.scenarios(variant):
            for key, cmd, answer in runs(variant, sc):
                data[sc["name"] + ".cmd" + key] = as_bytes(cmd)
                data[sc["name"] + ".out" + key] = as_bytes(answer)
            share = rc.ambiguous_share(sc)
            assert share <= rc.AMBIGUOUS_CAP, (variant, sc["name"], share)
            print("%-10s %-16s ambiguous share %.4f" % (variant, sc["name"], share))
        np.savez_compressed(path(variant), **data)
        print(path(variant), os.path.getsize(path(variant)), "bytes")


def _floats(records):
    out = []
    for name, v in records:
        if name == "state":
            out += [v["px"], v["py"], v["pz"], v["w"]]
        elif name == "fusion":
            out += [v["wsum"], v["guessed"]]
        elif name in ("voxel_to_pos", "pdf_table", "query_pdf", "forgetting_factor"):
            out.append(np.asarray(v).reshape(-1))
        elif name == "ring":
            out.append(v["map_center"])
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in out]) if out else np.zeros(0)


def spread():
    worst = 0.0
    for variant in ref_ring.VARIANTS:
        for sc in rc.scenarios(variant):
            a = runs(variant, sc, "O0")
            b = runs(variant, sc, "O3native")
            d = 0.0
            for (_, _, ta), (_, _, tb) in zip(a, b):
                fa, fb = _floats(ref_ring.parse(ta)), _floats(ref_ring.parse(tb))
                assert fa.shape == fb.shape, (variant, sc["name"])
                both = np.isfinite(fa) & np.isfinite(fb)
                d = max(d, float(np.abs(fa[both] - fb[both]).max()) if both.any() else 0.0)
            same = all(ta == tb for (_, _, ta), (_, _, tb) in zip(a, b))
            print("%-10s %-16s %s largest float difference %g, answers %s" % (variant, sc["name"], "exact " if sc["exact"] else "random", d,
                                                                           "identical" if same else "DIFFER"))
            worst = max(worst, d)
    print("largest difference over all scenarios: %g" % worst)


if __name__ == "__main__":
    spread() if "--spread" in sys.argv else write()
