"""SemanticDSPMap::worldReach / queryWorldReach / worldReachPaths (include/semantic_dsp_map.h): tests/cpp/adapter_world_reach.cpp
compiled against the stand-in Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, and on the GPU a
route is planned through the archive of a wall scene - results against the C ABI called directly, paths from goal to
start, a budget, the snapshot."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_reach", tmp_path / "adapter_world_reach")


def test_adapter_world_reach_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_reach_plans_through_the_archive(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world reach ok" in out.stdout, out.stdout + out.stderr
