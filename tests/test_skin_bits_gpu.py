"""The bits the FLAME skinning kernels and their operand packers return, as a recorded table.

The geometry tests compare the skinning forms with float64 within 5e-6 and the soak compares them with each other.  After the
split of csrc/flame.hip into csrc/lbs_skin.hip and csrc/lbs_tiles.h the split kernels (lbs_skin_bf16x3, the lbs_skin_v2 family)
SHARE their MFMA sequence and their `dirs` load, and every producer of a tile record (lbs_prepare, lbs_pack, lbs_tiles_f16)
shares one writer and one set of offsets.  A slip in a shared piece moves every form together: it stays inside the 5e-6
tolerances and inside the v2-against-bf16x3 soak.  This test holds each call to the SHA-256 of its outputs instead, on seeded
inputs generated on the host (the synthetic asset recipe of tests/test_geometry_gpu.py, NB = 150).

tests/golden/skin_bits.json was recorded from the library of the commit BEFORE that split: that commit's libmsmd_hip.so, built
beside this checkout and loaded through MSMD_LIB, ran this module's own recorder

    MSMD_LIB=<the parent's csrc/libmsmd_hip.so> python tests/test_skin_bits_gpu.py --record FILE

twice, with identical files (every launch writes all of every output hashed here: padding frames of the last tile record,
padding vertices of the dp planes and the padded vertex slot of an fp16 row included).  It is not an output of the code under
test.

Rows.  V = 130 (two 128-vertex tiles, an even V, padding pair lanes) at B = 1, 17, 65, 300 (the padding-frame and
padding-lane paths): lbs_prepare, lbs_pack, and every skinning form and the backward.  V = 5023, B = 2100, where the workgroup
cap bites: 22 frame splits of 96 frames = six tiles per workgroup -- prologue, steady state and drain of the 4-deep ring, three
two-tile barrier groups.  flame_prepare + lbs_skin_v2 at V = 130, B = 65, NS = 100, NE = 50 with every frame sharing the shape
row (the fold: flag, folded template, skipped K groups) and with one frame differing (the general path)."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmd_amd import _lib, ops  # noqa: E402
from test_geometry_gpu import KP, dev, lbs_inputs, model, rng  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skin_bits.json")
NB, NS, NE = 150, 100, 50
V_SMALL, BS_SMALL = 130, (1, 17, 65, 300)
V_LARGE, B_LARGE = 5023, 2100


def digest(*outs):
    h = hashlib.sha256()
    for t in outs:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def prepared(V, B):
    """(constants, coef, coef_hl, A, joints, tiles) of ops.lbs_prepare on the seeded inputs of (V, B): computed once, shared by
    the rows and left unchanged."""
    c = model(V, NB)[2]
    betas, pose = lbs_inputs(f"skin_bits/{V}/{B}", B, NB)
    return (c,) + tuple(ops.lbs_prepare(dev(betas), dev(pose), c.JS, c.parents, KP, want_split=True, want_blend_tiles=True))


def padded_rows(v16, V):
    """The fp16 vertices with the padded slot of each row, as tests/test_geometry_gpu.py reads it."""
    V_ld = V + (V & 1)
    return torch.as_strided(v16, (v16.shape[0], V_ld, 3), (V_ld * 3, 3, 1))


# ----------------------------------------------------------------------------- the calls
def prepare(V, B):
    return digest(*prepared(V, B)[1:])


def pack(V, B):
    _, coef, _, A, _, _ = prepared(V, B)
    return digest(*ops.lbs_pack(coef, A, want_split=True))


def skin(form, V, B):
    c, coef, coef_hl, A, _, tiles = prepared(V, B)
    v2 = (tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, V)
    if form == "fp32":
        return digest(ops.lbs_skin(coef, A, c.template_planes, c.dirs, c.weight_planes, V))
    if form == "bf16x3":
        return digest(ops.lbs_skin_bf16x3(coef_hl, A, c.template_planes, c.dirs_hl, c.weight_planes, V))
    if form == "v2 fp32":
        return digest(ops.lbs_skin_v2(*v2))
    if form == "v2 fp16 vertex-exact":
        return digest(padded_rows(ops.lbs_skin_v2(*v2, out_dtype=torch.float16), V))
    if form == "v2 fp16 planes":      # through msmd_lbs_tiles_f16
        return digest(padded_rows(ops.lbs_skin_v2(*v2, out_dtype=torch.float16, dirs_f16=c.dirs_f16), V))
    assert form == "v2 train"
    return digest(*ops.lbs_skin_v2_train(*v2))


def skin_bwd(V, B):
    c = model(V, NB)[2]
    g = rng(f"skin_bits/bwd/{V}/{B}")
    grad, p = g.standard_normal((B, V, 3)).astype(np.float32), (0.1 * g.standard_normal((B, V, 3))).astype(np.float32)
    A = g.standard_normal((B, 5, 12)).astype(np.float32)
    return digest(*ops.lbs_skin_bwd(dev(grad), dev(p), dev(A), c.weight_planes))


def flame(one_subject, V=V_SMALL, B=65):
    c = model(V, NB)[2]
    g = rng(f"skin_bits/flame/{one_subject}")
    shape = np.repeat((0.5 * g.standard_normal((1, NS))).astype(np.float32), B, 0)
    if not one_subject:
        shape[B // 2, 3] += 0.5
    expr, pose6 = (0.5 * g.standard_normal((B, NE))).astype(np.float32), (0.4 * g.standard_normal((B, 6))).astype(np.float32)
    tiles, flag, folded = ops.flame_prepare(dev(shape), dev(expr), dev(pose6), None, c.JS, c.parents, False, c.dirs, c.template_planes)
    verts = ops.lbs_skin_v2(tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, V, shape_varies=flag, folded=folded)
    assert (int(flag.item()) == 0) == one_subject
    return digest(tiles, flag, folded, verts)


def table():
    rows = {}
    for B in BS_SMALL:
        at = f"V {V_SMALL} B {B}"
        rows[f"lbs_prepare {at}"] = (prepare, V_SMALL, B)
        rows[f"lbs_pack {at}"] = (pack, V_SMALL, B)
        for form in ("fp32", "bf16x3", "v2 fp32", "v2 fp16 vertex-exact", "v2 fp16 planes", "v2 train"):
            rows[f"skin {form} {at}"] = (skin, form, V_SMALL, B)
        rows[f"lbs_skin_bwd {at}"] = (skin_bwd, V_SMALL, B)
    for form in ("bf16x3", "v2 fp32", "v2 fp16 planes", "v2 train"):
        rows[f"skin {form} V {V_LARGE} B {B_LARGE}"] = (skin, form, V_LARGE, B_LARGE)
    rows["flame_prepare + v2, one subject (fold)"] = (flame, True)
    rows["flame_prepare + v2, one frame differs"] = (flame, False)
    return rows


TABLE = table()


def run_row(name):
    f, *args = TABLE[name]
    return f(*args)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_the_table(recorded):
    assert sorted(recorded) == sorted(TABLE) and len(TABLE) == 42


@pytest.mark.parametrize("name", list(TABLE))
def test_skin_bits_are_the_recorded_ones(name, recorded):
    assert run_row(name) == recorded[name], f"{name}: the output bits differ from the parent commit's"


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_skin_bits_gpu.py --record FILE")
    print(f"recording the bits of {_lib.LIB_PATH}", file=sys.stderr)
    with open(sys.argv[2], "w") as out:
        json.dump({name: run_row(name) for name in TABLE}, out, indent=0, sort_keys=True)
        out.write("\n")
