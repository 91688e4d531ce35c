"""Times the two renderer launches (csrc/render.hip) on FLAME-sized input: V = 5023 vertices, a closed lat-long sphere of
F = 9976 faces (58 x 86; the vertices beyond the sphere's 4990 are in no face), B = 100 frames at 512 x 512 and 256 x 256.

HIP events around each launch, median of 9 after 3 warm-up rounds.  Prints one line per (size, launch) with the time, frames/s and
the bytes/s of what the launch stores (vertex stage: screen + normals; raster stage: RGBA8 + fp32 depth), and the pair's
frames/s.  Needs an MI355X; there is no CPU path.

    python tools/bench_render.py [--out profiles/r08_render.txt]

--texture N adds the textured shading pass with an N x N noise texture in longitude / latitude coordinates:
per size, the untextured raster launch, the textured pass alone and the two together, timed in turn within every round (so
the three share the clock state), per frame, and the textured pass with a 1 x 1 texture: the set-up, lighting and stores that
stage (C) of the raster launch also does for every covered pixel, which is wasted work under a texture.  --parent_lib PATH names another build of the library (the parent commit's,
the same C ABI): its msmd_render_raster and msmd_render_shade_textured are timed in the same rounds beside raw calls of this build's,
and each pair is reported as this build's median over the parent's with the parent's own spread over the rounds.

    python tools/bench_render.py --texture 1024 [--parent_lib /path/to/parent/libmsmd_hip.so] [--out profiles/r11_texture.txt]

--samples 4 times the four-sample raster launch instead: per size, the one-sample launch, the four-sample launch
and, with --parent_lib, the parent build's two launches, in turn within every round.

    python tools/bench_render.py --samples 4 [--parent_lib /path/to/parent/libmsmd_hip.so] [--out profiles/5_27_msaa.txt]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from msmd_amd import ops, synth  # noqa: E402
from msmd_amd.utils.renderer import MeshRenderer  # noqa: E402


def timed(fn, reps=9, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def timed_in_turn(fns, reps=9, warmup=3):
    """Medians (ms) of several launches timed one after the other within every round."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def parent_entry(path, name):
    """Entry point `name` of another build of the library: the same C ABI, so this build's prototypes."""
    from msmd_amd import _lib
    _lib.load()
    fn = getattr(ctypes.CDLL(path), name)
    fn.argtypes, fn.restype = _lib.PROTOS[name], ctypes.c_int
    return fn


def against_parent(what, mine, parent):
    """This build's median over the parent build's in the same rounds, beside the parent's own spread (max - min) / median."""
    return (f"{what}: this build / the parent's {mine[0] / parent[0]:.4f} (the parent's spread over its rounds "
            f"{(parent[2] - parent[1]) / parent[0]:.4f})")


def bench_texture(args, dev, v, f, verts, rot, tc, lines):
    from msmd_amd import _lib
    B, V = verts.shape[:2]
    N = args.texture
    img = torch.from_numpy(np.floor(synth.uniform01("bench_render/texture", N * N * 3) * np.float32(256)).astype(np.uint8)
                           .reshape(N, N, 3)).to(dev)
    pyramid = ops.texture_pyramid(img)
    pyramid1 = ops.texture_pyramid(img[:1, :1].contiguous())      # one texel: the pass without its texture traffic
    vt = np.stack([np.arctan2(v[:, 0], v[:, 2]) / (2 * np.pi) + 0.5, np.arcsin(np.clip(v[:, 1] / 0.09, -1, 1)) / np.pi + 0.5], axis=1)
    vt_d, ft_d = torch.from_numpy(vt.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev)
    lib = _lib.load()
    parent = parent_tex = None
    if args.parent_lib:
        parent = parent_entry(args.parent_lib, "msmd_render_raster")
        parent_tex = parent_entry(args.parent_lib, "msmd_render_shade_textured")
    for size in (512, 256):
        r = MeshRenderer((size, size))
        faces, off, ids = r._tables(torch.from_numpy(f).to(dev), V, dev)
        view, shade, lights = r._device_consts(dev)
        near, far = r.frustum["near"], r.frustum["far"]
        screen, normals = ops.render_vertices(verts, faces, off, ids, view, 1.0 / np.tan(r.fov / 2.0), size, size, tc, rot)
        rgba, depth, fid = ops.render_raster(screen, normals, faces, shade, lights, size, size, near, far, 0xffffffff, want_face_id=True)
        raster = lambda: ops.render_raster(screen, normals, faces, shade, lights, size, size, near, far, 0xffffffff, want_face_id=True)
        shade_t = lambda: ops.render_shade_textured(screen, normals, faces, vt_d, ft_d, pyramid, N, N, shade, lights, fid, rgba, near)
        both = lambda: (raster(), shade_t())
        shade_1 = lambda: ops.render_shade_textured(screen, normals, faces, vt_d, ft_d, pyramid1, 1, 1, shade, lights, fid, rgba, near)
        fns, names = [raster, shade_t, both], ["msmd_render_raster (untextured, with face ids)", "msmd_render_shade_textured",
                                               "raster + textured pass"]
        stream = torch.cuda.current_stream().cuda_stream
        raster_args = (screen.data_ptr(), normals.data_ptr(), faces.data_ptr(), shade.data_ptr(), lights.data_ptr(), lights.shape[0],
                       rgba.data_ptr(), depth.data_ptr(), fid.data_ptr(), B, V, faces.shape[0], size, size, near, far, 0xffffffff, stream)
        tex_args = (screen.data_ptr(), normals.data_ptr(), faces.data_ptr(), vt_d.data_ptr(), ft_d.data_ptr(), pyramid.data_ptr(), N, N,
                    shade.data_ptr(), lights.data_ptr(), lights.shape[0], fid.data_ptr(), rgba.data_ptr(), None, B, V, faces.shape[0],
                    vt_d.shape[0], size, size, near, stream)
        if parent is not None:
            fns.append(lambda: parent(*raster_args))
            names.append("parent build's msmd_render_raster")
        uvl = ops.render_shade_textured(screen, normals, faces, vt_d, ft_d, pyramid, N, N, shade, lights, fid, rgba, near, want_uvl=True)
        cov = fid >= 0
        lam = uvl[..., 2][cov]
        fns.append(shade_1)
        names.append("msmd_render_shade_textured with a 1 x 1 texture (set-up, lighting and stores: what stage (C) of the raster "
                     "launch repeats)")
        if parent is not None:        # raw calls of both builds on the same buffers: the same host work between the two events
            fns += [lambda: lib.msmd_render_raster(*raster_args), lambda: lib.msmd_render_shade_textured(*tex_args),
                    lambda: parent_tex(*tex_args)]
            names += ["msmd_render_raster, raw call", "msmd_render_shade_textured, raw call",
                      "parent build's msmd_render_shade_textured, raw call"]
        res = timed_in_turn(fns)
        for name, (med, lo, hi) in zip(names, res):
            lines.append(f"{name} B={B} {size}x{size} texture {N}x{N}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}, 9 rounds in "
                         f"turn), {med / B * 1e3:.2f} us / frame")
        lines.append(f"textured / untextured per frame {size}x{size}: {res[2][0] / res[0][0]:.3f}"
                     + (f"; against the parent build's untextured raster: {res[2][0] / res[3][0]:.3f} (this build's untextured raster / "
                        f"the parent's: {res[0][0] / res[3][0]:.3f})" if parent is not None else "")
                     + f"; {100 * float(cov.float().mean()):.1f} % of the pixels covered, mean level of detail {float(lam.mean()):.2f}; the "
                     f"untextured shading of those pixels inside the raster launch is wasted work under a texture")
        if parent is not None:
            lines.append(against_parent(f"msmd_render_raster {size}x{size}", res[-3], res[3]))
            lines.append(against_parent(f"msmd_render_shade_textured {size}x{size}", res[-2], res[-1]))


def bench_samples(args, dev, f, verts, rot, tc, lines):
    """One- and four-sample raster launches (and the parent build's) as raw calls of the C entry points on the same preallocated
    buffers, so that every launch carries the same host work between its two events."""
    from msmd_amd import _lib
    B, V = verts.shape[:2]
    lib = _lib.load()
    parent = parent_ms = None
    if args.parent_lib:
        parent = parent_entry(args.parent_lib, "msmd_render_raster")
        parent_ms = parent_entry(args.parent_lib, "msmd_render_raster_ms")
    for size in (512, 256):
        r = MeshRenderer((size, size))
        faces, off, ids = r._tables(torch.from_numpy(f).to(dev), V, dev)
        view, shade, lights = r._device_consts(dev)
        near, far = r.frustum["near"], r.frustum["far"]
        screen, normals = ops.render_vertices(verts, faces, off, ids, view, 1.0 / np.tan(r.fov / 2.0), size, size, tc, rot)
        rgba, depth, _ = ops.render_raster(screen, normals, faces, shade, lights, size, size, near, far, 0xffffffff)
        stream = torch.cuda.current_stream().cuda_stream
        head = (screen.data_ptr(), normals.data_ptr(), faces.data_ptr(), shade.data_ptr(), lights.data_ptr(), lights.shape[0],
                rgba.data_ptr(), depth.data_ptr())
        tail = (B, V, faces.shape[0], size, size, near, far, 0xffffffff)
        one = lambda: lib.msmd_render_raster(*head, None, *tail, stream)
        ms = lambda: lib.msmd_render_raster_ms(*head, None, None, *tail, args.samples, stream)
        fns, names = [one, ms], ["msmd_render_raster", f"msmd_render_raster_ms samples={args.samples}"]
        if parent is not None:
            fns += [lambda: parent(*head, None, *tail, stream), lambda: parent_ms(*head, None, None, *tail, args.samples, stream)]
            names += ["parent build's msmd_render_raster", f"parent build's msmd_render_raster_ms samples={args.samples}"]
        n = (ops.render_raster(screen, normals, faces, shade, lights, size, size, near, far, 0xffffffff, want_face_id=True,
                               samples=args.samples)[2] >= 0).sum(-1)
        res = timed_in_turn(fns)
        for name, (med, lo, hi) in zip(names, res):
            lines.append(f"{name} B={B} V={V} F={faces.shape[0]} {size}x{size}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}, 9 rounds "
                         f"in turn), {B / med * 1e3:.0f} frames/s")
        lines.append(f"{args.samples} samples / 1 sample {size}x{size}: {res[1][0] / res[0][0]:.3f}"
                     + (f"; this build's one-sample raster / the parent's: {res[0][0] / res[2][0]:.3f}" if parent is not None else "")
                     + f"; {100 * float((n > 0).float().mean()):.1f} % of the pixels have a covered sample, "
                     f"{100 * float(((n > 0) & (n < args.samples)).float().mean()):.2f} % are partly covered")
        if parent is not None:
            lines.append(against_parent(f"msmd_render_raster {size}x{size}", res[0], res[2]))
            lines.append(against_parent(f"msmd_render_raster_ms samples={args.samples} {size}x{size}", res[1], res[3]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--texture", type=int, default=0, help="side of a noise texture: time the textured pass too (0: do not)")
    ap.add_argument("--samples", type=int, default=1, choices=ops.RENDER_SAMPLES,
                    help="4: time the four-sample raster launch beside the one-sample launch instead")
    ap.add_argument("--parent_lib", type=str, default=None, help="another build of the library whose launches are timed in turn")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_render needs an MI355X"
    dev = torch.device("cuda:0")
    v, f = synth.latlong_sphere(58, 86, 0.09, n_vertices=synth.FLAME_V)
    B, V, Fc = args.frames, v.shape[0], f.shape[0]
    scale = 1.0 + 0.1 * np.arange(B, dtype=np.float32)[:, None, None] / B
    verts = torch.from_numpy(v[None] * scale).to(dev)
    rot = torch.from_numpy(0.3 * synth.normalish("bench_render/rot", (B, 3))).float().to(dev)
    tc = torch.zeros(3, device=dev)
    lines = []
    if args.samples != 1:
        bench_samples(args, dev, f, verts, rot, tc, lines)
    for size in (512, 256) if args.samples == 1 else ():
        r = MeshRenderer((size, size))
        faces, off, ids = r._tables(torch.from_numpy(f).to(dev), V, dev)
        view, shade, lights = r._device_consts(dev)
        focal = 1.0 / np.tan(r.fov / 2.0)
        vertex = lambda: ops.render_vertices(verts, faces, off, ids, view, focal, size, size, tc, rot)
        screen, normals = vertex()
        raster = lambda: ops.render_raster(screen, normals, faces, shade, lights, size, size, r.frustum["near"], r.frustum["far"],
                                           0xffffffff)
        depth = raster()[1]
        covered = float((depth > 0).float().mean())
        tv, tr = timed(vertex), timed(raster)
        for name, (med, lo, hi), nbytes in (("msmd_render_vertices", tv, B * V * 6 * 4), ("msmd_render_raster", tr, B * size * size * 8)):
            lines.append(f"{name} B={B} V={V} F={Fc} {size}x{size}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}, 9 runs), "
                         f"{B / med * 1e3:.0f} frames/s, {nbytes / med * 1e3 / 1e9:.2f} GB/s stored")
        lines.append(f"both launches {size}x{size}: {B / (tv[0] + tr[0]) * 1e3:.0f} frames/s, {100 * covered:.1f} % of the pixels covered")
    if args.texture > 0:
        bench_texture(args, dev, v, f, verts, rot, tc, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
