"""Times the two renderer launches (csrc/render.hip) on FLAME-sized input: V = 5023 vertices, a closed lat-long sphere of
F = 9976 faces (58 x 86; the vertices beyond the sphere's 4990 are in no face), B = 100 frames at 512 x 512 and 256 x 256.

HIP events around each launch, median of 9 after 3 warm-up rounds.  Prints one line per (size, launch) with the time, frames/s and
the bytes/s of what the launch stores (vertex stage: screen + normals; raster stage: RGBA8 + fp32 depth), and the pair's
frames/s.  Needs an MI355X; there is no CPU path.

    python tools/bench_render.py [--out profiles/r08_render.txt]
"""
import argparse
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", type=str, default=None)
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
    for size in (512, 256):
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
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
