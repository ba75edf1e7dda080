"""Registers, scratch and kernel sets of the nine derived-layer units (no GPU needed: the objects `build()` leaves in
csrc/ are taken apart like tests/test_isa_hygiene.py does).  The layers share their device code through sdm_layer.h and
sdm_walk.h; a change to a shared helper reaches every kernel that uses it, and the walking kernels are bound by latency,
so a wave of occupancy lost is time lost.  For every kernel: no scratch memory, no spilled vector register, no more
scalar registers spilled and no more vector registers allocated (in blocks of 8) than the ceiling; and every unit has
exactly the kernels listed.

The ceilings are constants: `vgpr_count` of each kernel in a build of commit 5095166 ("Add an on-device surface mesh
layer"), the last one in which every layer carried its own copy of that code, made with csrc/Makefile's flags.  In that
build the two k_ground_walk kernels spill 30 scalar registers each (into vector lanes, no scratch); every other kernel
spills none."""
import re
import subprocess
import os

import pytest

from tests.test_isa_hygiene import LLVM, device_elf, kernels_meta

VGPR_CEILING = {
    "queries": {
        "k_query_points": 10, "k_query_segments": 75, "k_query_boxes": 46,
    },
    "esdf": {
        "k_esdf_x": 26, "k_query_distance": 58, "k_esdf_env<1>": 48, "k_esdf_env<2>": 48,
    },
    "instances": {
        "k_instances_finalize": 83, "k_instances_accumulate<1>": 107, "k_instances_accumulate<0>": 54,
    },
    "frontiers": {
        "k_frontier_classify": 16, "k_frontier_mask": 32, "k_frontier_compact": 50, "k_frontier_accumulate": 49,
        "k_frontier_flags": 6, "k_frontier_table": 58, "k_frontier_label<1>": 16, "k_frontier_label<0>": 20,
    },
    "views": {
        "k_view_rays<0>": 88, "k_view_rays<1>": 54,
    },
    "reach": {
        "k_reach_seed": 10, "k_reach_list": 8, "k_reach_reduce": 10, "k_reach_relax<0,2,2,2>": 80,
        "k_reach_relax<0,2,2,3>": 80, "k_reach_relax<0,2,3,2>": 80, "k_reach_relax<0,2,3,3>": 80,
        "k_reach_relax<0,3,2,2>": 80, "k_reach_relax<0,3,2,3>": 80, "k_reach_relax<0,3,3,2>": 80,
        "k_reach_relax<0,3,3,3>": 123, "k_reach_relax<1,2,2,2>": 50, "k_reach_relax<1,2,2,3>": 54,
        "k_reach_relax<1,2,3,2>": 54, "k_reach_relax<1,2,3,3>": 56, "k_reach_relax<1,3,2,2>": 54,
        "k_reach_relax<1,3,2,3>": 56, "k_reach_relax<1,3,3,2>": 55, "k_reach_relax<1,3,3,3>": 63,
        "k_reach_classify<1>": 30, "k_reach_classify<0>": 23, "k_query_reach<1>": 43, "k_query_reach<0>": 68,
        "k_reach_paths<1>": 76, "k_reach_paths<0>": 79,
    },
    "forecast": {
        "k_forecast_classify": 31, "k_forecast_scatter": 31, "k_forecast_reduce": 8, "k_forecast_cells_count": 6,
        "k_forecast_cells_write": 8, "k_query_forecast": 13, "k_query_forecast_segments": 153,
    },
    "ground": {
        "k_ground_x": 58, "k_ground_rows": 70, "k_ground_cols": 23, "k_query_ground": 20, "k_query_footprints": 34,
        "k_ground_walk<1>": 49, "k_ground_walk<2>": 49,
    },
    "mesh": {
        "k_mesh_classify": 18, "k_mesh_faces": 70, "k_mesh_corner_count": 4, "k_mesh_emit": 96,
        "k_mesh_vertices": 24, "k_mesh_stats": 28,
    },
}
SGPR_SPILL_CEILING = {"k_ground_walk<1>": 30, "k_ground_walk<2>": 30}  # every other kernel: 0


def kernel_key(mangled):
    """k_name, or k_name<template arguments> (integers and bools as numbers), of a kernel of sdm's anonymous namespace"""
    m = re.match(r"_ZN3sdm12_GLOBAL__N_1(\d+)", mangled)
    assert m, mangled
    base, rest = mangled[m.end():m.end() + int(m.group(1))], mangled[m.end() + int(m.group(1)):]
    if not rest.startswith("I"):
        return base
    return "%s<%s>" % (base, ",".join(re.findall(r"L[bi](\d+)E", rest[1:rest.index("EEv") + 1])))


def sgpr_spills(elf):
    """mangled name -> sgpr_spill_count (kernels_meta does not keep it)"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+\.(name|sgpr_spill_count):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m:
            out[name] = int(m.group(2))
    return out


def allocated(vgpr_count):
    return -(-vgpr_count // 8) * 8


@pytest.mark.parametrize("unit", sorted(VGPR_CEILING))
def test_registers_scratch_and_kernels_of_a_layer(tmp_path, unit):
    elf = device_elf(tmp_path, unit)
    assert elf is not None
    meta, spills = kernels_meta(elf), sgpr_spills(elf)
    assert len(meta) == len(spills)
    got = {kernel_key(name): (v, spills[name]) for name, v in meta.items()}
    assert len(got) == len(meta) and sorted(got) == sorted(VGPR_CEILING[unit])
    for k, (v, sgpr_spilled) in sorted(got.items()):
        print(unit, k, "vgpr", v["vgpr_count"], "of", VGPR_CEILING[unit][k], "sgpr", v["sgpr_count"], "scratch", v["private_segment_fixed_size"])
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0, (k, v)
        assert sgpr_spilled <= SGPR_SPILL_CEILING.get(k, 0), (k, sgpr_spilled)
        assert allocated(int(v["vgpr_count"])) <= allocated(VGPR_CEILING[unit][k]), (k, v["vgpr_count"], VGPR_CEILING[unit][k])
