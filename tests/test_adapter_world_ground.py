"""SemanticDSPMap::worldGround / queryWorldGround / checkWorldFootprints (include/semantic_dsp_map.h):
tests/cpp/adapter_world_ground.cpp compiled against the stand-in Eigen/OpenCV/PCL headers and linked with libsdm_hip.so;
constructed here, and on the GPU the ground layer of the archive of a wall scene, the wall taken as the ground - the answers
against the C ABI called directly, one cell of height per cell walked away from the wall, a footprint of nine columns, the
snapshot under a worldRetain."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_ground", tmp_path / "adapter_world_ground")


def test_adapter_world_ground_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_ground_stands_on_the_wall(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world ground layer ok" in out.stdout, out.stdout + out.stderr
