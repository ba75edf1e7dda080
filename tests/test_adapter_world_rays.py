"""SemanticDSPMap::queryWorldSegments / scoreWorldViews (include/semantic_dsp_map.h): tests/cpp/adapter_world_rays.cpp
compiled against the stand-in Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, and on the GPU the
two members on the archive of a wall scene - the answers against the C ABI called directly, a ray toward the wall that hits
at the wall's cell, a ray away from it through bricks the archive does not have, a view toward the wall."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_rays", tmp_path / "adapter_world_rays")


def test_adapter_world_rays_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_rays_walks_the_archive(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world rays ok" in out.stdout, out.stdout + out.stderr
