"""The code object of the distance field (esdf.hip) keeps the hygiene tests/test_isa_hygiene.py enforces for the other
objects: no FLAT memory instructions, no scratch or spills in any of its kernels."""
import os
import re
import subprocess

from tests.test_isa_hygiene import LLVM, device_elf, kernels_meta

ESDF_KERNELS = ("k_esdf_x", "k_esdf_envILi1", "k_esdf_envILi2", "k_query_distance")


def test_esdf_object_has_no_flat_memory_instructions(tmp_path):
    elf = device_elf(tmp_path, "esdf")
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", elf], check=True, capture_output=True, text=True).stdout
    hits = [line for line in dis.splitlines() if re.search(r"\bflat_(load|store|atomic)", line)]
    assert not hits, hits[:5]
    for k in ESDF_KERNELS:
        assert k in dis, k


def test_esdf_kernels_use_no_scratch(tmp_path):
    meta = kernels_meta(device_elf(tmp_path, "esdf"))
    for k in ESDF_KERNELS:
        found = [v for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        assert int(found[0]["private_segment_fixed_size"]) == 0 and int(found[0]["vgpr_spill_count"]) == 0, (k, found)
