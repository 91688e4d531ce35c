"""Times the overlay operator (ops.draw_overlay, csrc/overlay.hip) on 64 frames of 1080 x 1920 x 3, in place:
  landmarks   per frame 478 discs of radius 1, one box outline, nine capsules (three arrows) and a 40-character line
  empty       no records at all: every workgroup reads its frame's two offsets and leaves
  scan        the same number of records per frame, all of them outside the frame: the cost of the per-tile scan alone
each at samples = 16 and samples = 1.  HIP events around a window of calls that lasts at least --window seconds, after --warmup
calls; the window's mean per call.  The share of HBM time is against reading and writing every frame once at 8.0 TB/s: that is
what the out-of-place form has to move; in place, untouched tiles move nothing, so the bound overstates what this run needs.

    python tools/bench_overlay.py [--frames 64] [--window 0.5] [--warmup 3] [--out FILE] [--once]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmd_amd import ops  # noqa: E402
from msmd_amd.utils import overlay as ov  # noqa: E402

HBM_PEAK = 8.0e12
H, W = 1080, 1920


def workload(n, outside=False):
    """-> the Overlay of the landmark workload; outside: every point moved 4 000 px left of the frame."""
    g = np.random.default_rng(7)
    shift = -4000.0 if outside else 0.0
    boxes = np.tile(np.array([[700.0 + shift, 250.0, 520.0, 600.0]]), (n, 1)) + g.uniform(-20, 20, (n, 4))
    pts = boxes[:, None, :2] + g.uniform(0, 1, (n, 478, 2)) * boxes[:, None, 2:]
    ypr = g.uniform(-30, 30, (n, 3))
    o = ov.landmark_overlay(pts)
    ov.box_overlay(boxes, into=o)
    ov.head_pose_overlay(ypr, boxes, into=o)                   # nine capsules and a line of 36 to 40 characters
    return o


def timed(fn, warmup, window):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    calls, total = 1, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        total = a.elapsed_time(b) * 1e-3
        if total >= window:
            return total / calls * 1e3, calls
        calls = max(calls * 2, int(calls * window / max(total, 1e-6) * 1.2) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--once", action="store_true", help="one call per case and no timing: the run a kernel trace is taken from")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    n = args.frames
    frames = torch.randint(0, 256, (n, H, W, 3), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(1))
    font = torch.from_numpy(np.array(ov.FONT)).to(dev)
    hbm_ms = 2 * frames.numel() / HBM_PEAK * 1e3
    cases = {"landmarks": workload(n).build(dev), "scan": workload(n, outside=True).build(dev),
             "empty": (torch.zeros(0, 8, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int32, device=dev))}
    lines = [f"overlay: {n} frames of {H} x {W} x 3 in place; {torch.cuda.get_device_name(0)}; tile {ops.OVERLAY_TILE_W} x "
             f"{ops.OVERLAY_TILE_H}, chunk {ops.OVERLAY_CHUNK}; mean of a window of at least {args.window} s after {args.warmup} calls; "
             f"reading and writing the frames once at 8.0 TB/s takes {hbm_ms:.3f} ms ({hbm_ms / n * 1e3:.2f} us per frame)"]
    for tag, (prims, offsets) in cases.items():
        per = prims.shape[0] / n
        for samples in (16, 1):
            fn = lambda: ops.draw_overlay(frames, prims, offsets, font, samples)
            if args.once:
                fn()
                torch.cuda.synchronize()
                continue
            ms, calls = timed(fn, args.warmup, args.window)
            lines.append(f"    {tag:10s} samples {samples:2d}  {per:6.1f} records per frame  {ms:8.3f} ms per call ({calls} calls)  "
                         f"{ms / n * 1e3:8.2f} us per frame  {ms / hbm_ms:6.2f} x the HBM time of one read and one write")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
