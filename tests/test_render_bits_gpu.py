"""The bits the renderer's entry points return (csrc/render.hip), as a recorded table.

The renderer tests compare the passes with numpy restatements "within one level" and under depth bounds.  The untextured, the textured
and the vertex-colour pass SHARE their barycentrics, their colour-to-bytes routine, the per-pixel resolve and (the two deferred passes)
their kernel and launcher: a slip in a shared piece moves all three together and stays inside those tolerances.  This
test holds each call chain to the SHA-256 of its outputs instead, on seeded inputs generated on the host: the meshes, rotations, frames
and cases of tests/test_render_msaa_gpu.py, the textures and coordinates of tests/test_texture_gpu.py and the colours of
tests/test_vertex_color_gpu.py, which are already the smallest shapes at which each path is taken.  No numpy reference runs here.

tests/golden/render_bits.json was recorded from the library of the commit BEFORE the pieces were shared (the C ABI is the same): that
commit's libmsmd_hip.so, built beside this checkout and loaded through MSMD_LIB, ran this module's own recorder

    MSMD_LIB=<the parent's csrc/libmsmd_hip.so> python tests/test_render_bits_gpu.py --record FILE

twice, with identical files.  It is not an output of the code under test.  Every hashed buffer is wholly written by its row's calls:
the raster pass stores every pixel of rgba, depth, face_id and sample_depth; a deferred pass starts from a copy of the same row's
raster rgba; uvl is stored at every pixel (zeros at a miss).

Rows.  Vertex stage: mesh `a`, B = 3 turned per frame about T_CENTER and B = 1 unturned.  Raster at one and at four samples: the seven
CASES of test_render_msaa_gpu under a white background (the 32 / 64 tile straddle, the wave walk, sub-pixel faces, the mid-stream
flush of the compacted list, an image edge one pixel past a tile edge), one case per sample count under a clear one, the `_ms` entry
at one sample (want_sample_depth), and `near` raised to NEAR_CUT so that the set-up drops part of mesh `b` (its unturned eye depths
are 1 - z: 0.90 .. 1.10, 531 of its 600 faces have a vertex nearer).  The texture pyramid.  The textured pass: meshes `a`, `b` at
37 x 53 B 3 and 130 x 70 B 1 with three textures, rgba and uvl at one sample, rgba at four, and one row without uvl.  Vertex colours:
shared and per frame, lit and unlit, one and four samples.  Rewound faces: every other face with corners 1 and 2 swapped (the construction of
test_vertex_color_gpu.test_rewound_faces_give_the_same_image, the texture coordinates swapped with their face), through both deferred
passes: "a face and its coordinates swap together"."""
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
from test_render_msaa_gpu import CASES, CLEAR, DEV, FAR, NEAR, T_CENTER, WHITE, case_id, frames, mesh, renderer, rots  # noqa: E402
from test_texture_gpu import mesh as uv_mesh, texture  # noqa: E402
from test_vertex_color_gpu import colours  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_bits.json")
NEAR_CUT = 1.0
CLEAR_CASE = NEAR_CASE = ("b", 64, 64, 1)
MS_ENTRY_CASE = ("b", 130, 70, 3)
DEFERRED = [(37, 53, 3), (130, 70, 1)]          # (W, H, B)
PYRAMIDS = ["1x1", "5x3", "64x32-rgba", "256x256"]
TEXTURES = ["5x3", "256x256", "64x32-rgba"]


def digest(*outs):
    h = hashlib.sha256()
    for t in outs:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def staged(name, W, H, B, turned=True):
    """(screen, normals, faces, shade, lights) of a case on the device: computed once, shared by the rows and left unchanged."""
    v, f = mesh(name)
    r = renderer(W, H)
    verts = dev(frames(v, B))
    faces_d, off, ids = r._tables(f, v.shape[0], verts.device)
    view, shade, lights = r._device_consts(verts.device)
    rot = rots(B) if turned else None
    screen, normals = ops.render_vertices(verts, faces_d, off, ids, view, 1.0 / np.tan(r.fov / 2.0), H, W,
                                          None if rot is None else dev(T_CENTER), None if rot is None else dev(rot))
    return screen, normals, faces_d, shade, lights


def raster_of(stage, W, H, S, faces=None, background=WHITE, near=NEAR, **kw):
    screen, normals, faces_d, shade, lights = stage
    return ops.render_raster(screen, normals, faces_d if faces is None else faces, shade, lights, H, W, near, FAR, background,
                             want_face_id=True, samples=S, **kw)


@functools.lru_cache(maxsize=None)
def rastered(name, W, H, B, S):
    """The raster pass a deferred row starts from: shared and left unchanged (the row shades a copy of rgba)."""
    return raster_of(staged(name, W, H, B), W, H, S)


# ----------------------------------------------------------------------------- the calls
def vertices(B):
    return digest(*staged("a", 37, 53, B, turned=B > 1)[:2])


def raster(case, S, background=WHITE, near=NEAR, ms_entry=False):
    name, W, H, B = case
    kw = dict(want_sample_depth=True) if S == 4 or ms_entry else {}
    return digest(*raster_of(staged(name, W, H, B), W, H, S, background=background, near=near, **kw))


def pyramid(name):
    return digest(ops.texture_pyramid(dev(texture(name))))


def textured(name, W, H, B, tex, S, want_uvl=True):
    screen, normals, faces_d, shade, lights = staged(name, W, H, B)
    _, _, vt, ft = uv_mesh(name)
    img = texture(tex)
    rgba, _, fid = rastered(name, W, H, B, S)
    rgba = rgba.clone()
    uvl = ops.render_shade_textured(screen, normals, faces_d, dev(vt), dev(ft), ops.texture_pyramid(dev(img)), img.shape[0],
                                    img.shape[1], shade, lights, fid, rgba, NEAR, want_uvl=want_uvl and S == 1, samples=S,
                                    background=WHITE)
    return digest(rgba) if uvl is None else digest(rgba, uvl)


def vertex_colour(name, kind, lit, S, W=37, H=53, B=3):
    screen, normals, faces_d, shade, lights = staged(name, W, H, B)
    rgba, _, fid = rastered(name, W, H, B, S)
    rgba = rgba.clone()
    ops.render_shade_vertex_color(screen, normals, faces_d, dev(colours(name, kind, B)), shade, lights, fid, rgba, NEAR, lit=lit,
                                  samples=S, background=WHITE)
    return digest(rgba)


def rewound(S, W=64, H=64):
    stage = staged("a", W, H, 1)                     # the normals of the list as it is: the passes under test do not depend on them
    screen, normals, _, shade, lights = stage
    v, f, vt, ft = uv_mesh("a")
    half, half_t = f.copy(), ft.copy()
    half[::2], half_t[::2] = half[::2][:, [0, 2, 1]], half_t[::2][:, [0, 2, 1]]
    fd, img = dev(half), texture("64x32-rgba")
    flat, depth, fid = raster_of(stage, W, H, S, faces=fd)
    tex, col = flat.clone(), flat.clone()
    ops.render_shade_textured(screen, normals, fd, dev(vt), dev(half_t), ops.texture_pyramid(dev(img)), img.shape[0], img.shape[1],
                              shade, lights, fid, tex, NEAR, samples=S, background=WHITE)
    ops.render_shade_vertex_color(screen, normals, fd, dev(colours("a", "shared", 1)), shade, lights, fid, col, NEAR, samples=S,
                                  background=WHITE)
    return digest(flat, depth, fid, tex, col)


def table():
    rows = {"vertices a B3 turned": (vertices, 3), "vertices a B1": (vertices, 1)}
    for S in (1, 4):
        for case in CASES:
            rows[f"raster S{S} {case_id(case)}"] = (raster, case, S)
        rows[f"raster S{S} {case_id(CLEAR_CASE)} clear background"] = (raster, CLEAR_CASE, S, CLEAR)
        for W, H, B in DEFERRED:
            for name in ("a", "b"):
                for tex in TEXTURES:
                    rows[f"textured S{S} {name}-{W}x{H}-B{B} {tex}"] = (textured, name, W, H, B, tex, S)
        for name in ("a", "b"):
            for kind in ("shared", "per_frame"):
                for lit in (True, False):
                    rows[f"vertex colour S{S} {name} {kind} {'lit' if lit else 'unlit'}"] = (vertex_colour, name, kind, lit, S)
        rows[f"rewound faces S{S}"] = (rewound, S)
    rows[f"raster S1 {case_id(MS_ENTRY_CASE)} through the _ms entry"] = (raster, MS_ENTRY_CASE, 1, WHITE, NEAR, True)
    rows[f"raster S1 {case_id(NEAR_CASE)} near {NEAR_CUT}"] = (raster, NEAR_CASE, 1, WHITE, NEAR_CUT)
    rows["textured S1 a-37x53-B3 256x256 without uvl"] = (textured, "a", 37, 53, 3, "256x256", 1, False)
    for name in PYRAMIDS:
        rows[f"pyramid {name}"] = (pyramid, name)
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
    assert sorted(recorded) == sorted(TABLE) and len(TABLE) == 67


@pytest.mark.parametrize("name", list(TABLE))
def test_render_bits_are_the_recorded_ones(name, recorded):
    assert run_row(name) == recorded[name], f"{name}: the output bits differ from the parent commit's"


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_render_bits_gpu.py --record FILE")
    print(f"recording the bits of {_lib.LIB_PATH}", file=sys.stderr)
    with open(sys.argv[2], "w") as out:
        json.dump({name: run_row(name) for name in TABLE}, out, indent=0, sort_keys=True)
        out.write("\n")
