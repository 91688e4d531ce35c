"""Times the JPEG encoder (csrc/jpeg.hip, ops.jpeg_encode) on what the renderer produces: B = 100 frames of 512 x 512 RGBA of a
lat-long sphere of FLAME's size (V = 5023, F = 9976), quality 90.

HIP events around `ops.jpeg_encode` (five launches and the one host read of the stream's length), median of 9 after 3 warm-up
rounds.  Prints the time, frames/s, the GB/s of pixels read and the MB written, the time of each entry point on its own, and
next to them the time of what the encoder replaces: the same frames copied to the host raw (`.cpu()`, pageable memory, as
`inference.main` does for `frames_*.npy`).  Needs an MI355X; there is no CPU path.

    python tools/bench_video.py [--out profiles/r09_video.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from msmd_amd import _lib, ops, synth  # noqa: E402
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
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_video needs an MI355X"
    dev = torch.device("cuda:0")
    v, f = synth.latlong_sphere(58, 86, 0.09, n_vertices=synth.FLAME_V)
    B, N, q = args.frames, args.size, args.quality
    scale = 1.0 + 0.1 * np.arange(B, dtype=np.float32)[:, None, None] / B
    verts = torch.from_numpy(v[None] * scale).to(dev)
    rot = torch.from_numpy(0.3 * synth.normalish("bench_render/rot", (B, 3))).float().to(dev)
    frames = MeshRenderer((N, N)).render_vertices(verts, f, t_center=np.zeros(3), rot=rot)[0]     # (B, N, N, 3) view of RGBA
    stream, offsets = ops.jpeg_encode(frames, q)
    out_mb = stream.numel() / 1e6
    in_bytes = B * N * N * 4
    lines = []
    med, lo, hi = timed(lambda: ops.jpeg_encode(frames, q))
    lines.append(f"ops.jpeg_encode B={B} {N}x{N} RGBA quality={q}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}, 9 runs), "
                 f"{B / med * 1e3:.0f} frames/s, {in_bytes / med * 1e3 / 1e9:.1f} GB/s of pixels read, {out_mb:.2f} MB written "
                 f"({in_bytes / 1e6 / out_mb:.1f} x smaller)")
    # the entry points on their own (the same buffers every time)
    lib = _lib.load()
    p = lambda t: t.data_ptr()
    n_int = lib.msmd_jpeg_intervals(N, N)
    header = torch.frombuffer(bytearray(ops.jpeg_header(N, N, q)), dtype=torch.uint8).to(dev)
    coef = torch.empty(B * n_int * 32 * 3 * 64, device=dev, dtype=torch.int16)
    ilen = torch.empty(B * n_int, device=dev, dtype=torch.int32)
    irel = torch.empty(B * n_int, device=dev, dtype=torch.int64)
    fsize = torch.empty(B, device=dev, dtype=torch.int64)
    offs = torch.empty(B + 1, device=dev, dtype=torch.int64)
    out = torch.empty_like(stream)
    sb, sh, sw, _ = frames.stride()
    st = lambda: torch.cuda.current_stream().cuda_stream
    steps = (("msmd_jpeg_coefficients", lambda: lib.msmd_jpeg_coefficients(p(frames), sb, sh, sw, B, N, N, q, p(coef), st())),
             ("msmd_jpeg_measure", lambda: lib.msmd_jpeg_measure(p(coef), B, N, N, header.numel(), p(ilen), p(irel), p(fsize), p(offs), st())),
             ("msmd_jpeg_write", lambda: lib.msmd_jpeg_write(p(coef), B, N, N, p(header), header.numel(), p(irel), p(offs), p(out),
                                                             out.numel(), st())))
    for name, fn in steps:
        med1, lo1, hi1 = timed(fn)
        lines.append(f"  {name}: median {med1:.4f} ms (min {lo1:.4f}, max {hi1:.4f})")
    assert torch.equal(out, stream) and torch.equal(offs, offsets)
    # what the encoder replaces: the raw frames to the host
    def raw():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames.cpu()
        return (time.perf_counter() - t0) * 1e3
    raw()
    raw_ms = float(np.median([raw() for _ in range(9)]))

    def packed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s, o = ops.jpeg_encode(frames, q)
        s.cpu(), o.cpu()
        return (time.perf_counter() - t0) * 1e3
    packed()
    packed_ms = float(np.median([packed() for _ in range(9)]))
    lines.append(f"frames to the host, wall clock, median of 9: raw (B, N, N, 3) .cpu() {raw_ms:.2f} ms ({B * N * N * 3 / 1e6:.0f} MB); "
                 f"encode + stream.cpu() {packed_ms:.2f} ms ({out_mb:.2f} MB)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
