"""The kernels of the world match (world_match.hip) are exactly the ones DESIGN.md 5u names, use no scratch, spill no vector
and no scalar register, stay within 128 VGPRs, and the scoring kernel's LDS is what 5u states.  Reads the code object's
metadata only.  (tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit.)"""
import os
import re

from tests.abi_checks import ROOT
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

WORLD_MATCH_KERNELS = ("k_wmt_score", "k_wmt_reduce")
# the window's two row planes [24][24] words, its label bytes [24][24][24], the source brick's two planes of eight 64-bit
# layers, its list of up to 512 occupied cells (two bytes each), 64 pool slots and one flag, in steps of the planes' 8 bytes
SCORE_LDS = (2 * 24 * 24 * 4 + 24 * 24 * 24 + 2 * 8 * 8 + 512 * 2 + 64 * 4 + 4 + 7) // 8 * 8
REDUCE_LDS = 256 * (8 + 4 + 4)


def test_the_unit_is_listed():
    assert "world_match" in hip_units()


def test_design_names_the_kernels_and_the_lds():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("\n## 5u. ") + 1:]
    section = section[:section.index("\n## ")]
    assert sorted(set(re.findall(r"\bk_wmt_\w+", section))) == sorted(WORLD_MATCH_KERNELS)
    assert SCORE_LDS == 19848 and "19,848" in section and "4,096" in section


def test_world_match_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_match")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_MATCH_KERNELS), list(meta)   # (none of world_io.hip's: its launcher is a host function)
    want_lds = dict(k_wmt_score=SCORE_LDS, k_wmt_reduce=REDUCE_LDS)
    for k in WORLD_MATCH_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128 and lds[name] == want_lds[k], (k, v["vgpr_count"], lds[name])
