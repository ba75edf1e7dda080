"""SemanticDSPMap::worldMatch (include/semantic_dsp_map.h): tests/cpp/adapter_world_match.cpp compiled against the stand-in
Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, and on the GPU one map's archive of a wall scene is
imported into a second map under a planted offset, which worldMatch on the second finds again."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_match", tmp_path / "adapter_world_match")


def test_adapter_world_match_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_match_finds_a_planted_offset(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world match ok" in out.stdout, out.stdout + out.stderr
