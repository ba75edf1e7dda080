"""Registers, scratch and kernel sets of the nine derived-layer units (no GPU needed: the objects `build()` leaves in
csrc/ are taken apart like tests/test_isa_hygiene.py does).  The layers share their device code through sdm_layer.h and
sdm_walk.h; a change to a shared helper reaches every kernel that uses it, and the walking kernels are bound by latency,
so a wave of occupancy lost is time lost.  For every kernel: no scratch memory, no spilled vector register, no more
scalar registers spilled and no more vector registers allocated (in blocks of 8) than the ceiling; and every unit has
exactly the kernels listed.

The ceilings are constants: `vgpr_count` of each kernel in a build of commit 5095166 ("Add an on-device surface mesh
layer"), the last one in which every layer carried its own copy of that code, made with csrc/Makefile's flags.  In that
build the two k_ground_walk kernels spill 30 scalar registers each (into vector lanes, no scratch); every other kernel
spills none.

On the GPU: the layers with a scan (frontiers, mesh, world, forecast) run it on one scratch that the map owns
(layer_scan_scratch); `test_layers_share_the_scan_scratch` interleaves them on one map, with scans of both forms of
exclusive_scan_u32, and holds every output to that of a map that ran the one call alone."""
import re
import subprocess
import os

import numpy as np
import pytest

from semantic_dsp_map_amd import binding, synth
from tests import primitives_cases as pc
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


# ---- one scan scratch for the layers ---------------------------------------------------------------------------------
def _fed_map(cfg, params, frames):
    """a fresh map after the frames, nothing waited for: the layers' builds follow in stream order"""
    g = binding.SdmMap(cfg, params, synth.noise_table())
    for f in frames:
        g.update(*f)
    return g


def _filled(*arrays):
    """the bytes of the arrays, none of them empty"""
    assert all(len(a) > 0 for a in arrays), [len(a) for a in arrays]
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def _frontiers_out(g):
    table, origin = g.frontiers()
    return _filled(table, origin, *g.frontier_cells())


def _mesh_out(g):
    m = g.mesh()
    return _filled(np.atleast_1d(m["info"]), m["origin"], m["faces"], m["quads"], m["corners"], m["xyz"])


def _world_out(g):
    bricks, cells = g.world_bricks()
    return _filled(np.atleast_1d(g.world_info()), bricks, cells)


def _world_occupied_out(g):
    points, n = g.world_occupied()
    assert n == len(points)
    return _filled(points)


@pytest.mark.gpu
def test_layers_share_the_scan_scratch():
    """2^21 cells is the smallest map on which a layer's scan takes the two-launch form: the frontiers' flag scan over
    max_cells + 1 entries at max_cells = V; at the default capacity, V / 16, it is one launch like every other scan of
    the four layers.  One map runs the layers' calls interleaved on the shared scratch, and every output equals, byte for
    byte, that of a fresh map which was fed the same frames and ran that call alone.  (Three frames, like the large case of
    tests/test_frontiers_gpu.py: after one frame no cell of this map reads occupied, and mesh, archive and forecast would
    be empty.)"""
    cfg, params, frames = synth.make_frames("C2", 3)
    V = 1 << (cfg["x_n"] + cfg["y_n"] + cfg["z_n"])
    assert V == 1 << 21 and not pc.one_launch(V + 1) and pc.one_launch(V // 16 + 1) and pc.one_launch((V >> 6) + 1)
    motions = np.zeros(4, binding.MOTION)   # the scene's four moving boxes
    motions["track"], motions["v"] = [1, 2, 3, 4], [[0.0, 0.0, 1.5], [0.0, 0.0, -1.0], [0.5, 0.0, 1.0], [0.0, 0.0, 2.0]]
    horizons = [0.5, 1.0, 2.0]

    a = _fed_map(cfg, params, frames)
    a.frontiers_update(max_cells=V)               # 1: a two-launch flag scan
    a.mesh_update()                               # 2
    a.world_update()                              # 3
    a.forecast_update(motions, horizons)          # 4
    forecast_a = _filled(*a.forecast_cells())
    frontiers_1, mesh_2 = _frontiers_out(a), _mesh_out(a)
    a.frontiers_update(max_cells=0)               # 5: a one-launch flag scan behind the two-launch one's totals
    occupied_a = _world_occupied_out(a)           # 6
    frontiers_5, world_a = _frontiers_out(a), _world_out(a)
    a.frontiers_update(max_cells=V)               # 7
    a.mesh_update()                               # 8
    frontiers_7, mesh_8 = _frontiers_out(a), _mesh_out(a)
    a.close()

    g = _fed_map(cfg, params, frames)
    g.frontiers_update(max_cells=V)
    frontiers_alone = _frontiers_out(g)
    g.close()
    g = _fed_map(cfg, params, frames)
    g.mesh_update()
    mesh_alone = _mesh_out(g)
    g.close()
    g = _fed_map(cfg, params, frames)
    g.world_update()
    world_alone, occupied_alone = _world_out(g), _world_occupied_out(g)
    g.close()
    g = _fed_map(cfg, params, frames)
    g.forecast_update(motions, horizons)
    forecast_alone = _filled(*g.forecast_cells())
    g.close()

    assert frontiers_1 == frontiers_alone and frontiers_7 == frontiers_alone and frontiers_1 == frontiers_7
    # (the frontier cells fit the default capacity, so table and cells are those of the longer list)
    assert len(frontiers_alone[2]) // 4 <= V // 16 and frontiers_5 == frontiers_alone
    assert mesh_2 == mesh_alone and mesh_8 == mesh_alone and mesh_2 == mesh_8
    assert world_a == world_alone and occupied_a == occupied_alone
    assert forecast_a == forecast_alone
