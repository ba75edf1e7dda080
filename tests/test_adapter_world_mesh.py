"""SemanticDSPMap::worldMesh (include/semantic_dsp_map.h): tests/cpp/adapter_world_mesh.cpp compiled against the stand-in
Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, and on the GPU the mesh of the archive of a wall
scene - the lists against the C ABI called directly, the normals, the closed mesh, a cap, a box, the snapshot under a
worldRetain."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_mesh", tmp_path / "adapter_world_mesh")


def test_adapter_world_mesh_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_mesh_meshes_the_wall(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world mesh ok" in out.stdout, out.stdout + out.stderr
