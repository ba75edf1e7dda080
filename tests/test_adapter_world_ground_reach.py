"""SemanticDSPMap::worldGroundReach / queryWorldGroundReach / worldGroundReachPaths (include/semantic_dsp_map.h):
tests/cpp/adapter_world_ground_reach.cpp compiled against the stand-in Eigen/OpenCV/PCL headers and linked with
libsdm_hip.so; constructed here, and on the GPU the field over the ground layer of a wall scene's archive, the wall taken as
the ground - the answers against the C ABI called directly, the cost's closed form on the flat wall and paths as long as it
says, every path cell on ground, the snapshot under a worldRetain that empties the archive."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_ground_reach", tmp_path / "adapter_world_ground_reach")


def test_adapter_world_ground_reach_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_ground_reach_drives_over_the_wall(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world ground reach ok" in out.stdout, out.stdout + out.stderr
