"""What the built gfx950 code objects must not contain (no GPU needed: the objects `build()` leaves in csrc/ are taken
apart with the LLVM tools of the ROCm image).  Round 4 found three things in the ISA that the source did not show and
that each cost dependent memory round trips (last bullet group); they stay out:

  * FLAT memory instructions (a pointer whose address space the compiler cannot see: every later wait becomes
    `vmcnt(0) lgkmcnt(0)`),
  * scratch memory in the replay of the moved copies (a conditional operator on two struct lvalues selects an address),
  * more than 128 registers in the dense sweep (fewer than four waves per SIMD).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semantic_dsp_map_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def hip_units():
    """Every .hip unit of the library, from the one place that lists them (SRCS in csrc/Makefile): a unit cannot be added
    without being scanned."""
    m = re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    return [f[:-len(".hip")] for f in m.group(1).split()]


def device_elf(tmp_path, name):
    """The gfx950 code object inside csrc/<name>.o; None if the unit has no device code (host code only)."""
    obj = os.path.join(CSRC, name + ".o")
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump", "llvm-readelf")]
    if not os.path.exists(obj) or not all(os.path.exists(t) for t in tools):
        pytest.skip("no built object / no LLVM tools here (run __graft_entry__.build() first)")
    sections = subprocess.run([tools[3], "-S", obj], check=True, capture_output=True, text=True).stdout
    if ".hip_fatbin" not in sections:
        return None
    fat = str(tmp_path / (name + ".fat"))
    elf = str(tmp_path / (name + ".elf"))
    subprocess.run([tools[0], "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + elf], check=True)
    return elf


def kernels_meta(elf):
    """name -> {vgpr_count, private_segment_fixed_size, ...} from the code object's notes"""
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    meta, cur = {}, {}
    for line in out.splitlines():
        m = re.match(r"\s+\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k in cur:  # the next kernel's block begins
            meta[cur["name"]] = cur
            cur = {}
        cur[k] = v
    if "name" in cur:
        meta[cur["name"]] = cur
    return meta


@pytest.mark.parametrize("name", hip_units())
def test_no_flat_memory_instructions(tmp_path, name):
    elf = device_elf(tmp_path, name)
    if elf is None:  # host code only: nothing to scan
        return
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", elf], check=True, capture_output=True, text=True).stdout
    cur, hits = None, {}
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            cur = m.group(1)
        elif re.search(r"\bflat_(load|store|atomic)", line):
            hits[cur] = hits.get(cur, 0) + 1
    assert not hits, "FLAT memory instructions in: %r" % hits


def test_registers_and_scratch_of_the_kernels_that_were_fixed(tmp_path):
    k = kernels_meta(device_elf(tmp_path, "kernels"))
    m = kernels_meta(device_elf(tmp_path, "moves"))
    dense = [v for n, v in k.items() if "k_occupancy_denseILi8" in n]
    assert len(dense) == 1 and int(dense[0]["vgpr_count"]) <= 128 and int(dense[0]["vgpr_spill_count"]) == 0, dense
    scan = [v for n, v in k.items() if "k_occupancy_scanILi8" in n]
    assert len(scan) == 1 and int(scan[0]["vgpr_count"]) <= 64 and int(scan[0]["vgpr_spill_count"]) == 0, scan
    for s in (2, 4, 8):
        rp = [v for n, v in m.items() if "k_move_replayILi%dE" % s in n]
        assert len(rp) == 1 and int(rp[0]["private_segment_fixed_size"]) == 0, (s, rp)


def test_the_tools_are_where_the_test_looks_for_them():
    # (a ROCm image without its LLVM tools would turn the two tests above into skips without anybody noticing)
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no ROCm toolchain in this environment")
    for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump", "llvm-readelf"):
        assert os.path.exists(os.path.join(LLVM, t)), t
