"""Times the JPEG decoder (csrc/jpeg_decode.hip, ops.jpeg_decode) on files of this project's encoder: B = 100 frames of 512 x 512
of the lat-long sphere `tools/bench_video.py` renders, quality 90, restart interval 32 (128 intervals a frame).

`ops.jpeg_decode` is timed by the wall clock around the call and a synchronise, median of 9 after 3 warm-up rounds: it parses on
the host, uploads five arrays and launches a fill and three kernels, so the host part is in the figure and is also printed on
its own (`ops._jpeg_plan`).  The three entry points are timed on resident buffers with HIP events.  The same frames re-written by
Pillow (4:4:4, quality 90, no restart markers) are the one-lane-per-frame case the decoder does not make fast.  Needs an MI355X.

    python tools/bench_decode.py [--out profiles/r11_decode.txt]
"""
import argparse
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from msmd_amd import _lib, ops, synth  # noqa: E402
from msmd_amd.utils import media  # noqa: E402
from msmd_amd.utils.renderer import MeshRenderer  # noqa: E402


def events(fn, reps=9, warmup=3):
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


def wall(fn, reps=9, warmup=3, sync=True):
    ms = []
    for k in range(warmup + reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def report(name, files, lines, dev):
    B = len(files)
    mb = sum(len(f) for f in files) / 1e6
    plan = ops._jpeg_plan(files)
    n_rows = int((plan.intervals[:, 1] >> 32 >= 0).sum())
    med, lo, hi = wall(lambda: ops.jpeg_decode(files, strict=False))
    lines.append(f"{name}: B={B} {plan.H}x{plan.W} layout={plan.layout}, {mb:.2f} MB read, {n_rows} intervals (lanes), {plan.n_sets} table set(s)")
    lines.append(f"  ops.jpeg_decode (host parse + uploads + launches): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}, 9 runs), "
                 f"{B / med * 1e3:.0f} frames/s")
    med, lo, hi = wall(lambda: ops._jpeg_plan(files), sync=False)
    lines.append(f"  host parse and tables alone (ops._jpeg_plan): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    lib = _lib.load()
    p = lambda t: t.data_ptr()
    st = lambda: torch.cuda.current_stream().cuda_stream
    stream, rows, sets, frame_set, status = ops._jpeg_upload(plan, dev)
    coef = torch.empty(B, plan.blocks, 64, device=dev, dtype=torch.int16)
    planes = torch.empty(B, plan.blocks * 64, device=dev, dtype=torch.uint8)
    px = torch.empty(B, plan.H, plan.W, 3, device=dev, dtype=torch.uint8)
    px4 = torch.empty(B, plan.H, plan.W, 4, device=dev, dtype=torch.uint8)
    steps = (("msmd_jpeg_decode_coefficients (fill + entropy decode)",
              lambda: lib.msmd_jpeg_decode_coefficients(p(stream), stream.numel(), p(rows), rows.shape[0], p(sets), plan.n_sets, B, plan.H,
                                                        plan.W, plan.layout, plan.ri, p(coef), p(status), st())),
             ("msmd_jpeg_decode_planes", lambda: lib.msmd_jpeg_decode_planes(p(coef), p(sets), plan.n_sets, p(frame_set), B, plan.H, plan.W,
                                                                            plan.layout, p(planes), st())),
             ("msmd_jpeg_decode_pixels, 3 channels", lambda: lib.msmd_jpeg_decode_pixels(p(planes), B, plan.H, plan.W, plan.layout, 3, p(px), st())),
             ("msmd_jpeg_decode_pixels, 4 channels", lambda: lib.msmd_jpeg_decode_pixels(p(planes), B, plan.H, plan.W, plan.layout, 4, p(px4), st())))
    for step, fn in steps:
        med, lo, hi = events(fn)
        lines.append(f"  {step}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})")
    assert int(status.abs().max()) == 0
    assert torch.equal(px, ops.jpeg_decode(files)) and torch.equal(px4[..., :3], px)
    return px


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_decode needs an MI355X"
    from PIL import Image
    dev = torch.device("cuda:0")
    v, f = synth.latlong_sphere(58, 86, 0.09, n_vertices=synth.FLAME_V)
    B, N, q = args.frames, args.size, args.quality
    scale = 1.0 + 0.1 * np.arange(B, dtype=np.float32)[:, None, None] / B
    verts = torch.from_numpy(v[None] * scale).to(dev)
    rot = torch.from_numpy(0.3 * synth.normalish("bench_render/rot", (B, 3))).float().to(dev)
    frames = MeshRenderer((N, N)).render_vertices(verts, f, t_center=np.zeros(3), rot=rot)[0]
    own = media.encode_jpeg(frames, q)
    lines = []
    px = report(f"own encoder, quality {q}, restart interval {ops.JPEG_RESTART_INTERVAL}", own, lines, dev)
    host = px.cpu().numpy()
    rewritten = []
    for b in range(B):
        buf = io.BytesIO()
        Image.fromarray(host[b]).save(buf, "JPEG", quality=q, subsampling=0)
        rewritten.append(buf.getvalue())
    report(f"the same frames re-written by Pillow, quality {q}, 4:4:4, no restart markers (one lane per frame)", rewritten, lines, dev)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
