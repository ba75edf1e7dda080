"""SemanticDSPMap::worldBricks / worldImport / worldRetain (include/semantic_dsp_map.h): tests/cpp/adapter_world_io.cpp
compiled against the stand-in Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, and on the GPU one
map's archive of a wall scene is handed to a second map - at offset 0, with FILL, moved by an offset - and trimmed, the
trim compared with the C ABI called directly."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_io", tmp_path / "adapter_world_io")


def test_adapter_world_io_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_io_hands_an_archive_to_a_second_map(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world io ok" in out.stdout, out.stdout + out.stderr
