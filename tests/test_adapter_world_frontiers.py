"""SemanticDSPMap::worldFrontiers (include/semantic_dsp_map.h): tests/cpp/adapter_world_frontiers.cpp compiled against the
stand-in Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, and on the GPU the frontier clusters of
the archive of a wall scene - the table against the C ABI called directly, its entries' consistency, inside_bricks and
min_cells, a cluster's first cell reached by worldReach(), the snapshot."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_frontiers", tmp_path / "adapter_world_frontiers")


def test_adapter_world_frontiers_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_frontiers_lists_where_to_go(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world frontiers ok" in out.stdout, out.stdout + out.stderr
