"""TEST INFRASTRUCTURE: the one command line that builds a program of tests/cpp/ - include/semantic_dsp_map.h compiled
against the stand-in Eigen/OpenCV/PCL headers of tests/mock_includes/ and linked with libsdm_hip.so."""
import os
import subprocess

from semantic_dsp_map_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_adapter(name, exe, defs=()):
    """tests/cpp/<name>.cpp -> the program `exe` (a path), with the -D options of `defs`; returns exe"""
    csrc = os.path.dirname(binding.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + list(defs) +
                          ["-I", os.path.join(ROOT, "tests", "mock_includes"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe), "-L", csrc, "-lsdm_hip",
                           "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)
