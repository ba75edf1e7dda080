"""Writes tests/golden/ref_filter_<variant>.npz: for every scenario of tests/ref_filter_cases.py the commands given to the
reference's filter harness (oracle/ref_filter_harness.cpp over the reference's own updateParticles, birth members and
resampleParticlesInVoxel) and the text it answered.

Needs the executables of `make -C oracle ref`, hence a checkout of the reference; the tests need only the fixtures.

    python -m tests.golden.make_golden_ref_filter            # write the fixtures, print the order spreads
    python -m tests.golden.make_golden_ref_filter --spread   # after `make -C oracle ref-spread`: the float spread between
                                                             # an -O0 and an -O3 -march=native build of the harness
"""
import os
import sys

import numpy as np

from oracle import ref_filter
from tests import ref_filter_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))


def path(variant):
    return os.path.join(HERE, "ref_filter_%s.npz" % variant)


def runs(variant, sc, flavour=None):
    """[(key, commands, answer)] of a scenario"""
    out, answers = [], {}
    while True:                             # two_frames: a later run is written from what the earlier ones answered
        todo = [(k, t) for k, t in fc.scripts(sc, answers).items() if k not in answers]
        if not todo:
            return out
        for key, text in todo:
            answers[key] = ref_filter.run(variant, text, flavour)
            out.append((key, text, answers[key]))


def as_bytes(text):
    return np.frombuffer(text.encode("ascii"), np.uint8)


def write():
    for variant in ref_filter.VARIANTS:
        data = {}
        for sc in fc.scenarios(variant):
            got = runs(variant, sc)
            for key, cmd, answer in got:
                if not key:             # the runs "o1", "o2" differ from it in the argument of permute_bins alone: scripts() writes them
                    data[sc["name"] + ".cmd"] = as_bytes(cmd)
                data[sc["name"] + ".out" + key] = as_bytes(answer)
            note = ""
            if len(got) > 1 and sc["kind"] == "frame":
                worst, differ = fc.order_spread([ref_filter.parse(a) for _, _, a in got])
                n = len(ref_filter.first(ref_filter.parse(got[0][2]), "particles", 0)["idx"])
                share = len(differ) / max(n, 1)
                assert share <= fc.AMBIGUOUS_CAP, (variant, sc["name"], share)
                note = "order spread %.3e (relative), integers that differ among the orders %d of %d" % (worst, len(differ), n)
            print("%-10s %-26s %s" % (variant, sc["name"], note))
        np.savez_compressed(path(variant), **data)
        print(path(variant), os.path.getsize(path(variant)), "bytes")


def _floats(records):
    out = []
    for name, v in records:
        if name == "particles":
            out += [v["px"], v["py"], v["pz"], v["w"]]
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in out]) if out else np.zeros(0)


def spread():
    worst = 0.0
    for variant in ref_filter.VARIANTS:
        for sc in fc.scenarios(variant):
            a = runs(variant, sc, "O0")
            b = runs(variant, sc, "O3native")
            d = 0.0
            for (_, _, ta), (_, _, tb) in zip(a, b):
                fa, fb = _floats(ref_filter.parse(ta)), _floats(ref_filter.parse(tb))
                assert fa.shape == fb.shape, (variant, sc["name"])
                both = np.isfinite(fa) & np.isfinite(fb)
                d = max(d, float(np.abs(fa[both] - fb[both]).max()) if both.any() else 0.0)
            same = all(ta == tb for (_, _, ta), (_, _, tb) in zip(a, b))
            print("%-10s %-26s %s largest float difference %g, answers %s" % (variant, sc["name"], "exact " if sc["exact"] else "order ", d,
                                                                           "identical" if same else "DIFFER"))
            worst = max(worst, d)
    print("largest difference over all scenarios: %g" % worst)


if __name__ == "__main__":
    spread() if "--spread" in sys.argv else write()
