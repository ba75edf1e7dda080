"""tests/instances_ref.py (the NumPy restatement the GPU tests compare the instance table with) against a brute-force
Python loop over all cells, on small hand-made result arrays with a shifted ring; and the layout of the INSTANCE dtype
against the order of the fields in include/sdm.h."""
import os
import re
import struct

import numpy as np
import pytest

from semantic_dsp_map_amd import binding
from tests import instances_ref as ir
from tests import query_ref as qr

CFG = dict(x_n=3, y_n=2, z_n=3, voxel_size=0.25)
RING = dict(map_center=[1.5, -0.25, 7.75], eq_steps=[5, 3, 6])
MAX_MOVABLE = 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def brute(cfg, ring, voxels, max_movable, flags):
    """cell by cell in map-index order, Python numbers only (floats rounded to float32 after every operation)"""
    N = [1 << cfg["x_n"], 1 << cfg["y_n"], 1 << cfg["z_n"]]
    size = f32(cfg["voxel_size"])
    origin = [f32(f32(ring["map_center"][a]) + f32(-f32(f32(N[a] >> 1) * size))) for a in range(3)]
    acc, labels = {}, [0] * 256
    for k in range(N[2]):
        for j in range(N[1]):
            for i in range(N[0]):
                r = [(c + e) % n for c, e, n in zip((i, j, k), ring["eq_steps"], N)]
                v = voxels[r[0] | (r[1] << cfg["x_n"]) | (r[2] << (cfg["x_n"] + cfg["y_n"]))]
                occ, t = int(v["occ"]), int(v["track"])
                if occ < 1 or ((flags & 2) and occ != 1) or ((flags & 1) and not 1 <= t <= max_movable):
                    continue
                labels[int(v["label"])] += 1
                a = acc.setdefault(t, dict(cells=[], labels=[], guessed=0, w=[]))
                a["cells"].append((i, j, k))
                a["labels"].append(int(v["label"]))
                a["guessed"] += occ == 2
                a["w"].append(float(v["wsum"]))
    out = []
    for t in sorted(acc):
        a = acc[t]
        c = a["cells"]
        e = dict(track=t, label=a["labels"][0], mixed_labels=int(len(set(a["labels"])) > 1), n_cells=len(c), n_guessed=a["guessed"],
                 first_cell=c[0][0] | (c[0][1] << cfg["x_n"]) | (c[0][2] << (cfg["x_n"] + cfg["y_n"])), wsum_max=max(a["w"]), pad=0)
        e["cell_min"] = [min(p[ax] for p in c) for ax in range(3)]
        e["cell_max"] = [max(p[ax] for p in c) for ax in range(3)]
        e["cell_sum"] = [sum(p[ax] for p in c) for ax in range(3)]
        e["cell_sq"] = [sum(p[u] * p[w] for p in c) for u, w in [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]]
        e["box_min"] = [f32(origin[ax] + f32(f32(e["cell_min"][ax]) * size)) for ax in range(3)]
        e["box_max"] = [f32(origin[ax] + f32(f32(e["cell_max"][ax] + 1) * size)) for ax in range(3)]
        e["centroid"] = [f32(origin[ax] + (e["cell_sum"][ax] / len(c) + 0.5) * size) for ax in range(3)]
        out.append(e)
    return out, labels


def crafted():
    """a result array in STORAGE order whose instances, seen in map-index cells, are: track 7 one cell in the corner
    (7, 3, 7); track 3 with cells on both sides of the wrap point of every axis; tracks 200 and 201 sharing label 9; track 5
    with labels 4 and 6; guessed cells on tracks 3 and 200; track 0 occupied; plus free and unknown cells carrying
    track ids that must not count"""
    geo = qr.Geometry(CFG, RING)
    V = 1 << (CFG["x_n"] + CFG["y_n"] + CFG["z_n"])
    vox = np.zeros(V, binding.VOXEL_RESULT)
    vox["occ"][::3] = -1
    vox["wsum"][::3] = -1
    vox["track"][1::3] = 3       # free cells with a track id
    grid = geo.voxel_grid()

    def put(i, j, k, track, label, occ, w):
        vox[grid[k, j, i]] = (w, track, label, occ)

    put(7, 3, 7, 7, 2, 1, 0.5)
    # storage index = map index + eq (mod N): map x 2 | 3 are storage 7 | 0, map y 0 | 1 storage 3 | 0, map z 1 | 2 storage 7 | 0
    for n, (i, j, k) in enumerate([(2, 0, 1), (3, 0, 1), (2, 1, 1), (3, 1, 2), (2, 0, 2), (4, 1, 2)]):
        put(i, j, k, 3, 11, 2 if n == 4 else 1, 0.25 + n)
    put(0, 0, 0, 200, 9, 1, 1.0)
    put(1, 0, 0, 200, 9, 2, 3.0)
    put(0, 2, 4, 201, 9, 1, 2.0)
    put(5, 2, 3, 5, 6, 1, 0.75)
    put(5, 2, 5, 5, 4, 1, 0.8)
    put(6, 3, 0, 0, 1, 1, 0.3)
    put(6, 3, 1, 0, 1, 1, 0.2)
    return geo, vox


@pytest.mark.parametrize("flags", ir.ALL_FLAGS)
def test_restatement_against_the_loop(flags):
    geo, vox = crafted()
    got = ir.instances(geo, vox, MAX_MOVABLE, CFG["voxel_size"], flags)
    ref, ref_labels = brute(CFG, RING, vox, MAX_MOVABLE, flags)
    assert len(got) == len(ref) and list(got["track"]) == [e["track"] for e in ref]
    for g, e in zip(got, ref):
        for k in binding.INSTANCE.names:
            want = np.array(e[k], binding.INSTANCE[k].base).reshape(binding.INSTANCE[k].shape)
            assert np.array_equal(np.asarray(g[k]), want), (flags, e["track"], k, g[k], e[k])
    assert list(ir.label_cells(geo, vox, MAX_MOVABLE, flags)) == ref_labels
    assert ir.equal_tables(got, got.copy()) is None


def test_the_crafted_cases_are_what_they_claim():
    geo, vox = crafted()
    t = {int(e["track"]): e for e in ir.instances(geo, vox, MAX_MOVABLE, CFG["voxel_size"], 0)}
    assert sorted(t) == [0, 3, 5, 7, 200, 201]
    assert list(t[7]["cell_min"]) == [7, 3, 7] == list(t[7]["cell_max"]) and t[7]["n_cells"] == 1
    # track 3 straddles the wrap point of every axis: its storage-order box spans the whole ring there
    lo, hi = ir.storage_box(geo, vox, MAX_MOVABLE, 0, 3)
    assert list(t[3]["cell_min"]) == [2, 0, 1] and list(t[3]["cell_max"]) == [4, 1, 2]
    assert list(lo) == [0, 0, 0] and list(hi) == [7, 3, 7]
    assert t[3]["n_guessed"] == 1 and t[200]["n_guessed"] == 1 and t[3]["first_cell"] == 2 | (0 << 3) | (1 << 5)
    assert t[200]["label"] == t[201]["label"] == 9 and not t[200]["mixed_labels"]
    assert t[5]["mixed_labels"] == 1 and t[5]["label"] == 6
    assert t[3]["wsum_max"] == np.float32(5.25)
    mov = ir.instances(geo, vox, MAX_MOVABLE, CFG["voxel_size"], ir.MOVABLE_ONLY)
    assert list(mov["track"]) == [3, 5, 7]
    obs = {int(e["track"]): e for e in ir.instances(geo, vox, MAX_MOVABLE, CFG["voxel_size"], ir.OBSERVED_ONLY)}
    assert obs[3]["n_cells"] == 5 and obs[3]["n_guessed"] == 0 and obs[200]["n_cells"] == 1
    assert ir.label_cells(geo, vox, MAX_MOVABLE, 0)[9] == 3 and ir.label_cells(geo, vox, MAX_MOVABLE, ir.OBSERVED_ONLY)[9] == 2
    # an empty selection is an empty table
    assert len(ir.instances(geo, np.zeros_like(vox), MAX_MOVABLE, CFG["voxel_size"], 0)) == 0
    assert ir.equal_tables(mov, mov[:2]) is not None


def test_dtype_matches_the_header():
    assert binding.INSTANCE.itemsize == 144
    text = open(os.path.join(ROOT, "include", "sdm.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sdm_instance;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = dict(uint8_t=1, uint16_t=2, uint32_t=4, uint64_t=8, float=4)
    off, fields = 0, []
    for ctype, name, count in re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body):
        off = (off + size[ctype] - 1) // size[ctype] * size[ctype]       # natural alignment
        fields.append((name, off, size[ctype] * int(count or 1)))
        off += size[ctype] * int(count or 1)
    assert off == 144
    assert [f[0] for f in fields] == list(binding.INSTANCE.names)
    for name, o, nbytes in fields:
        assert binding.INSTANCE.fields[name][1] == o and binding.INSTANCE.fields[name][0].itemsize == nbytes, name
    assert binding.INSTANCES_MOVABLE_ONLY == 1 and binding.INSTANCES_OBSERVED_ONLY == 2
    assert "#define SDM_INSTANCES_MOVABLE_ONLY  0x1u" in text and "#define SDM_INSTANCES_OBSERVED_ONLY 0x2u" in text
