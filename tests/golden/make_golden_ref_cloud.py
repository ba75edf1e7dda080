"""Writes tests/golden/ref_cloud_<variant>.npz: for every scenario of tests/ref_cloud_cases.py what the reference
harness (oracle/ref_cloud_harness.cpp over the reference's own generateLabeledPointCloud) answered, as the arrays of
oracle.ref_cloud.FIELDS under "<scenario>.<field>", and under "<scenario>.inputs" the SHA-256 of the scenario file it
was given.  The inputs themselves are not stored: the tests regenerate them from the seeds.

Needs the executables of `make -C oracle ref`, hence a checkout of the reference; the tests need only the fixtures.

    python -m tests.golden.make_golden_ref_cloud            # write the fixtures
    python -m tests.golden.make_golden_ref_cloud --spread   # after `make -C oracle ref-spread`: the largest difference
                                                            # between an -O0 and an -O3 -march=native build of the harness
"""
import os
import sys

import numpy as np

from oracle import ref_cloud
from tests import ref_cloud_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
SIZE_LIMIT = 212604     # the largest fixture before these (ref_ring_t1.npz)


def path(variant):
    return os.path.join(HERE, "ref_cloud_%s.npz" % variant)


def answer(variant, sc, flavour=None):
    """(scenario file, {field: array}) of a scenario"""
    text = ref_cloud.script(sc)
    return text, ref_cloud.parse(ref_cloud.run(variant, text, flavour))


def write():
    for variant in ref_cloud.VARIANTS:
        data = {}
        for sc in cc.scenarios(variant):
            text, rec = answer(variant, sc)
            cc.check_hits(sc, rec)
            data[sc["name"] + ".inputs"] = cc.inputs_hash(text)
            for k in ref_cloud.FIELDS:
                data[sc["name"] + "." + k] = rec[k]
            print("%-7s %-24s %5d valid, %4d clipped" % (variant, sc["name"], len(rec["pixel"]), int(rec["clipped"].sum())))
        np.savez_compressed(path(variant), **data)
        size = os.path.getsize(path(variant))
        print(path(variant), size, "bytes")
        assert size <= SIZE_LIMIT, size


def spread():
    worst = 0.0
    for variant in ref_cloud.VARIANTS:
        for sc in cc.scenarios(variant):
            _, a = answer(variant, sc, "O0")
            _, b = answer(variant, sc, "O3native")
            same = all(np.array_equal(a[k], b[k]) for k in ref_cloud.FIELDS if k not in ("pos", "sigma", "depth"))
            same = same and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("pos", "sigma", "depth"))
            d = float(np.abs(a["pos"].astype(np.float64) - b["pos"].astype(np.float64)).max()) if same or a["pos"].shape == b["pos"].shape else np.inf
            d = max(d, float(np.abs(a["sigma"].astype(np.float64) - b["sigma"].astype(np.float64)).max()) if a["sigma"].shape == b["sigma"].shape else np.inf)
            print("%-7s %-24s %s largest float difference %g, answers %s" % (variant, sc["name"], "exact " if sc["exact"] else "random", d,
                                                                          "identical" if same else "DIFFER"))
            worst = max(worst, d)
    print("largest difference over all scenarios: %g" % worst)


if __name__ == "__main__":
    spread() if "--spread" in sys.argv else write()
