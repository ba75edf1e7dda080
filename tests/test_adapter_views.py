"""SemanticDSPMap::scoreViews (include/semantic_dsp_map.h): tests/cpp/adapter_views.cpp compiled against the stand-in
Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, driven through a wall scene with one movable
object on the GPU and compared there with the C ABI called directly."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_views", tmp_path / "adapter_views")


def test_adapter_views_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_views_on_a_wall_scene(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "views ok" in out.stdout, out.stdout + out.stderr
