"""SemanticDSPMap::worldEsdf / queryWorldDistance (include/semantic_dsp_map.h): tests/cpp/adapter_world_esdf.cpp compiled
against the stand-in Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, and on the GPU the distance
field of the archive of a wall scene - the answers against the C ABI called directly, one voxel of distance per cell walked
away from the wall, "far" behind the radius, the snapshot under a worldRetain."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_esdf", tmp_path / "adapter_world_esdf")


def test_adapter_world_esdf_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_esdf_measures_the_clearance(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world distance field ok" in out.stdout, out.stdout + out.stderr
