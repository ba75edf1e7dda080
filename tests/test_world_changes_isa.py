"""The kernels of the world changes (world_changes.hip) are exactly those DESIGN.md 5y names, use no scratch, spill no vector
and no scalar register and stay within 128 VGPRs; the comparison and the brick-local labelling hold their words, keys, labels
and neighbour masks in registers - no LDS - and only the per-label counters use any, as 5y states.  Reads the code object's
metadata only.  (tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of the
library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills
from tests.test_world_frontiers_isa import lds_bytes

WORLD_CHANGES_KERNELS = ("k_wc_mark", "k_wc_index", "k_wc_compact", "k_wc_label_localILb0", "k_wc_label_localILb1", "k_wc_seamsILb0",
                         "k_wc_seamsILb1", "k_wc_roots", "k_wc_accumulate", "k_wc_flags", "k_wc_table", "k_wc_assign", "k_query_world_changes")
LDS_BYTES = {"k_wc_assign": 3072}      # three times 256 label counts a workgroup; every other kernel none


def test_the_unit_is_listed():
    assert "world_changes" in hip_units()


def test_world_changes_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "world_changes")
    meta, spills, lds = kernels_meta(elf), sgpr_spills(elf), lds_bytes(elf)
    assert len(meta) == len(WORLD_CHANGES_KERNELS), list(meta)   # (no kernel of the frame, none of another world unit)
    for k in WORLD_CHANGES_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        print(k, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"], "sgpr spilled", spills[name], "scratch", v["private_segment_fixed_size"], "lds",
              lds[name])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0 and spills[name] == 0, (k, v)
        assert int(v["vgpr_count"]) <= 128, (k, v["vgpr_count"])
        assert lds[name] == LDS_BYTES.get(k, 0), (k, lds[name])
