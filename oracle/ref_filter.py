"""Python side of oracle/ref_filter_harness.cpp: the commands it adds to those of oracle/ref_harness.cpp.

TEST INFRASTRUCTURE ONLY.  The executables are the reference's own filter members - updateParticles, the three birth
members and resampleParticlesInVoxel of semantic_dsp_map.h over ObjectParticleHashMap - compiled over oracle/ref_shims/
(`make -C oracle ref`, which needs a checkout of the reference).  Scenario, result and the records they hold are those of
oracle/ref_ring.py, which parses the new ones (births, resample, cursor, owners) too.
"""
import os

import numpy as np

from oracle import ref_ring
from oracle.ref_ring import VARIANTS, first, parse  # noqa: F401  (one surface for the tests)

_HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_KEYS = ("detection_probability", "noise_number", "nb_ptc_num_per_point", "occupancy_threshold", "max_obersevation_lost_time",
              "forgetting_rate", "max_forget_count", "match_score_threshold", "id_transition_probability", "if_consider_depth_noise",
              "if_use_independent_filter", "depth_noise_first_order", "depth_noise_zero_order")
_INT_PARAMS = ("nb_ptc_num_per_point", "max_obersevation_lost_time", "max_forget_count", "if_consider_depth_noise", "if_use_independent_filter")


def exe(variant, flavour=None):
    """path of the filter harness of a variant (flavour: None, "O0" or "O3native" of `make ref-spread`)"""
    if flavour:
        return os.path.join(_HERE, "_ref", "spread", "ref_filter_%s_%s" % (variant, flavour))
    return os.path.join(_HERE, "_ref", "ref_filter_" + variant)


def run(variant, text, flavour=None):
    return ref_ring.run(variant, text, path=exe(variant, flavour))


class Script(ref_ring.Script):
    def params(self, p):
        """setMapParameters, setMapOptions and setDepthNoiseModelParameters with every value of the dict"""
        self.lines.append("params " + " ".join(str(int(p[k])) if k in _INT_PARAMS else ref_ring.fhex(p[k]) for k in PARAM_KEYS))

    def cloud(self, default_sigma, rows):
        """rows: (row, col, x, y, z, sigma, label, track, valid); every other pixel is invalid with default_sigma"""
        self.lines.append("cloud %s %d" % (ref_ring.fhex(default_sigma), len(rows)))
        for r, c, x, y, z, sigma, label, track, valid in rows:
            self.lines.append(" %d %d %s %d %d %d" % (r, c, ref_ring._fl([x, y, z, sigma]), label, track, 1 if valid else 0))

    def set_owners(self, owners):
        self.lines.append("set_owners %d" % len(owners))
        for track in sorted(owners):
            self.lines.append(" %d %d %s" % (track, len(owners[track]), " ".join(str(int(i)) for i in owners[track])))

    def permute_bins(self, k):
        self.lines.append("permute_bins %d" % k)

    def update_particles(self):
        self.lines.append("update_particles")

    def births(self, mode=-1):
        self.lines.append("births %d" % mode)

    def resample(self, voxels):
        self.lines.append("resample %d %s" % (len(voxels), " ".join(str(int(v)) for v in voxels)))

    def guessed(self, pts, label, track):
        p = np.asarray(pts, np.float32).reshape(-1, 3)
        self.lines.append("guessed %d %d %d %s" % (label, track, len(p), ref_ring._fl(p)))

    def burn(self, n):
        self.lines.append("burn %d" % n)
