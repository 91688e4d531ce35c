"""Times the kernels of DESIGN.md 5.30 beside their siblings, raw calls of the C entry points on preallocated buffers:

  shading   msmd_render_shade_vertex_color (lit and unlit, shared and per-frame colours) against msmd_render_shade_textured[_ms] with a
            256 x 256 texture, on the face ids of one raster launch: FLAME topology (synth.flame_asset: 5023 vertices, 9976 faces),
            B = 64 frames at 512 x 512, one and four samples per pixel;
  colours   msmd_vertex_error_colors against msmd_vertex_frame_errors at n = 512, V = 5023, fp32 and fp16; msmd_vertex_error_sums and
            msmd_colormap_f64 beside them.

The launches of a group are timed in turn within every round (so they share the clock state): HIP events around `--launches` launches
of one kernel, 9 rounds after 3 warm-up rounds, the median per launch with the least and the greatest.  Needs an MI355X.

    python tools/bench_vertex_color.py [--out profiles/5_30_vertex_color.txt]

--parent_lib PATH names another build of the library (the parent commit's, the same C ABI): its shading passes are timed in the same
rounds, and each is reported as this build's median over the parent's with the parent's own spread (max - min) / median.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from msmd_amd import _lib, ops, synth  # noqa: E402
from msmd_amd.utils.metrics import colormap_table  # noqa: E402
from msmd_amd.utils.renderer import MeshRenderer  # noqa: E402


def timed_in_turn(fns, launches, reps=9, warmup=3):
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / launches)
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def report(lines, names, res, unit_bytes=None):
    for k, (name, (med, lo, hi)) in enumerate(zip(names, res)):
        rate = "" if unit_bytes is None else f", {unit_bytes[k] / med / 1e9:.2f} TB/s of the bytes the algorithm needs"
        lines.append(f"  {name}: median {med:.4f} ms per launch (min {lo:.4f}, max {hi:.4f}){rate}")


def bench_shading(args, dev, lines):
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    a = synth.flame_asset()
    v, f = a["v_template"].astype(np.float32), a["f"].astype(np.int32)
    B, V, size = args.frames, v.shape[0], args.size
    verts = torch.from_numpy(np.stack([v * np.float32(1.0 + 0.001 * b) for b in range(B)])).to(dev)
    rot = torch.from_numpy((0.3 * synth.normalish("bench_vertex_color/rot", (B, 3))).astype(np.float32)).to(dev)
    tc = torch.zeros(3, device=dev)
    N = 256
    img = torch.from_numpy(np.floor(synth.uniform01("bench_vertex_color/texture", N * N * 3) * np.float32(256)).astype(np.uint8)
                           .reshape(N, N, 3)).to(dev)
    pyramid = ops.texture_pyramid(img)
    vt = torch.from_numpy(synth.uniform("bench_vertex_color/vt", (V, 2), 0.0, 1.0)).to(dev)
    ft = torch.from_numpy(f).to(dev)
    shared = torch.from_numpy(np.floor(synth.uniform01("bench_vertex_color/vcol", B * V * 4) * np.float32(256)).astype(np.uint8)
                              .reshape(B, V, 4)).to(dev)
    for S in (1, 4):
        r = MeshRenderer((size, size), samples=S)
        faces, off, ids = r._tables(ft, V, dev)
        view, shade, lights = r._device_consts(dev)
        near, far = r.frustum["near"], r.frustum["far"]
        screen, normals = ops.render_vertices(verts, faces, off, ids, view, 1.0 / np.tan(r.fov / 2.0), size, size, tc, rot)
        rgba, _, fid = ops.render_raster(screen, normals, faces, shade, lights, size, size, near, far, 0xffffffff, want_face_id=True, samples=S)
        p = lambda t: t.data_ptr()
        tex = lambda L: (lambda: L.msmd_render_shade_textured_ms(p(screen), p(normals), p(faces), p(vt), p(ft), p(pyramid), N, N, p(shade),
                                                                 p(lights), lights.shape[0], p(fid), p(rgba), B, V, faces.shape[0], V, size,
                                                                 size, near, 0xffffffff, S, st))
        col = lambda L, table, per_frame, lit: (lambda: L.msmd_render_shade_vertex_color(
            p(screen), p(normals), p(faces), p(table), per_frame, lit, p(shade), p(lights), lights.shape[0], p(fid), p(rgba), B, V,
            faces.shape[0], size, size, near, 0xffffffff, S, st))
        passes = lambda L: [tex(L), col(L, shared[0], 0, 1), col(L, shared[0], 0, 0), col(L, shared, 1, 1), col(L, shared, 1, 0)]
        fns = passes(lib)
        names = [f"msmd_render_shade_textured{'_ms' if S == 4 else ''} ({N} x {N} texture)", "vertex colours, shared table, lit",
                 "vertex colours, shared table, unlit", "vertex colours, per-frame tables, lit", "vertex colours, per-frame tables, unlit"]
        if args.parent_lib:
            parent = ctypes.CDLL(args.parent_lib)
            for name in ("msmd_render_shade_textured_ms", "msmd_render_shade_vertex_color"):
                getattr(parent, name).argtypes, getattr(parent, name).restype = _lib.PROTOS[name], ctypes.c_int
            fns += passes(parent)
            names += [f"parent build's {name}" for name in names]
        assert all(fn() == 0 for fn in fns)
        res = timed_in_turn(fns, args.launches)
        cov = float((fid >= 0).float().mean())
        lines.append(f"shading passes, B = {B} frames of {size} x {size}, {S} sample(s) per pixel, V = {V}, F = {faces.shape[0]}, "
                     f"{100 * cov:.1f} % of the samples covered:")
        report(lines, names, res)
        lines.append(f"  vertex colours (shared, lit) / textured: {res[1][0] / res[0][0]:.3f}; unlit / lit: {res[2][0] / res[1][0]:.3f}; "
                     f"per-frame / shared (lit): {res[3][0] / res[1][0]:.3f}")
        for k in range(5 if args.parent_lib else 0):
            mine, theirs = res[k], res[5 + k]
            lines.append(f"  {names[k]}: this build / the parent's {mine[0] / theirs[0]:.4f} (the parent's spread over its rounds "
                         f"{(theirs[2] - theirs[1]) / theirs[0]:.4f})")


def bench_colours(args, dev, lines):
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    n, V = args.n, 5023
    g = torch.Generator(device="cpu").manual_seed(5)
    lut = torch.from_numpy(colormap_table("jet")).to(dev)
    region = torch.zeros(V, dtype=torch.uint8, device=dev)
    region[1000:1200] = 1
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    for dt, code in ((torch.float32, ops.F32), (torch.float16, ops.F16)):
        gt = (0.1 * torch.randn(n, V, 3, generator=g)).to(dt).to(dev)
        pred = (gt.float() + 0.002 * torch.randn(n, V, 3, generator=g).to(dev)).to(dt)
        table = torch.empty(n, 4, device=dev, dtype=torch.float64)
        out = torch.empty(n, V, 4, device=dev, dtype=torch.uint8)
        state = torch.zeros(1, V, device=dev, dtype=torch.float64)
        x = torch.rand(n * V, generator=g, dtype=torch.float64).to(dev)
        p = lambda t: t.data_ptr()
        fns = [lambda: lib.msmd_vertex_frame_errors(p(pred), p(gt), p(region), p(table), n, V, code, st),
               lambda: lib.msmd_vertex_error_colors(p(pred), p(gt), p(lut), p(out), n, V, code, 0.01, 0xffff00ff, st),
               lambda: lib.msmd_vertex_error_sums(p(pred), p(gt), 0, n, p(off), 1, p(state), V, code, st),
               lambda: lib.msmd_colormap_f64(p(x), p(lut), p(out), n * V, 1.0, 0xffff00ff, st)]
        names = ["msmd_vertex_frame_errors", "msmd_vertex_error_colors", "msmd_vertex_error_sums (one clip)", "msmd_colormap_f64 (n V values)"]
        assert all(fn() == 0 for fn in fns)
        read = 2 * n * V * 3 * pred.element_size()
        need = [read + V + 32 * n, read + 4 * n * V + 1024, read + 16 * V, 8 * n * V + 4 * n * V + 1024]
        res = timed_in_turn(fns, args.launches)
        lines.append(f"error field, n = {n} frames, V = {V}, {str(dt).split('.')[-1]}:")
        report(lines, names, res, need)
        lines.append(f"  msmd_vertex_error_colors / msmd_vertex_frame_errors: {res[1][0] / res[0][0]:.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--launches", type=int, default=20, help="launches of one kernel between two events")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--parent_lib", type=str, default=None, help="another build of the library whose shading passes are timed in turn")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    lines = [f"tools/bench_vertex_color.py on {torch.cuda.get_device_name(0)}: {args.launches} launches per window, 9 rounds in turn after 3 warm-up rounds"]
    bench_shading(args, dev, lines)
    bench_colours(args, dev, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
