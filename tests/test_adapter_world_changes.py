"""SemanticDSPMap::worldChanges / queryWorldChanges (include/semantic_dsp_map.h): tests/cpp/adapter_world_changes.cpp
compiled against the stand-in Eigen/OpenCV/PCL headers and linked with libsdm_hip.so; constructed here, and on the GPU the
changes between the block and the archive of a wall scene - none right after an archiving, the counters' sums and the
table's consistency once the block has seen more, the query at a region's first cell, all-zero masks, the snapshot and the
empty second build after the archiving."""
import subprocess

import pytest

from tests.adapter_build import build_adapter


def build_exe(tmp_path):
    return build_adapter("adapter_world_changes", tmp_path / "adapter_world_changes")


def test_adapter_world_changes_compiles_and_links(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adapter constructed" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_adapter_world_changes_finds_what_differs_from_the_archive(tmp_path):
    out = subprocess.run([build_exe(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "world changes ok" in out.stdout, out.stdout + out.stderr
